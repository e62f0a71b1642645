// Reverberation and additive noise on the GPU: what Kaldi's wav-reverberate does to one utterance, on a packed batch.
//
// Kaldi is not part of the reference tree (its recipes call the binary through the wav.scp pipelines that
// reverberate_data_dir.py and augment_data_dir.py write): **parity unpinned**.  The rule below restates wav-reverberate.cc as
// published and is the specification; include/xvec_hip.h repeats it and tests/helpers/ref_reverb.py states it in float64 numpy.
//
// An utterance has int16 samples x[0..N), N >= 1, at sample rate fs; optionally an impulse response h[0..L) = int16 / 32768
// (exact in float32), 1 <= L <= 65536; J >= 0 additive signals v_j[0..M_j) with snr_j in dB, a start time t_j in seconds and an
// extended length M'_j >= 1 (M'_j = M_j unless the signal came from a nested --duration pipe).  All rates are equal.
//
//  1. P_before = (sum x^2) / N.
//  2. With an RIR: y[n] = sum_k h[k] x[n - k] for n in [0, N + L - 1).  p = the lowest index of the largest *signed* h
//     (Vector::Max).  b = trunc(0.001 fs), a = trunc(0.05 fs); the early window is [s, e) = [max(0, p - b), min(L, p + a));
//     E = sum_n e[n]^2 / (N + (e - s) - 1), e = the same convolution restricted to the taps in [s, e).
//     Without an RIR: y = x, E = P_before, p = 0.  Y = len(y).
//  3. For j in order: P_j = sum_{i < M'_j} v_j[i mod M_j]^2 / M'_j, g_j = sqrt(10^(-snr_j / 10) E / P_j), o_j = trunc(t_j fs);
//     for 0 <= i < min(M'_j, Y - o_j): y[o_j + i] += g_j v_j[i mod M_j].  P_j = 0 is an error of that utterance (status 1);
//     no inf is ever written.
//  4. P_after = sum y^2 / Y.
//  5. scale = volume if volume > 0; else sqrt(P_before / P_after) if normalize_output (P_after = 0: status 2); else 1.
//  6. shift = p if there is an RIR and shift_output, else 0.  n_out = trunc(duration fs) if duration > 0, else N if
//     shift_output, else Y.  out[i] = scale y[(i + shift) mod Y] for i < n_out: the plain range when n_out <= N, the full tail
//     when shift_output = false, and the repetition that fills a --duration longer than the signal.
//  7. int16 output: trunc toward zero, then saturation to [-32768, 32767]; the saturated samples are counted per utterance.
//  8. Sums of squares and every scalar (E, P_*, g_j, scale) are double; partial sums are added in a fixed order, one per
//     workgroup, then a second fixed-order pass (the idiom of calibrate.hip); no floating-point atomics.  y is float32.  An
//     utterance's outputs are a pure function of its own inputs: the same bits on every repeat, alone or in any batch, and
//     for every legal workspace size (the tiling of an utterance depends on its own N, L and n_out alone, and the workspace
//     layout on the tables alone).
//
// Without an RIR the kernels run rule 2 with L = 1, h = [1]: y = x exactly, the window is [0, 1) and E = sum x^2 / N.
//
// Kernels, all on the caller's stream, in this order:
//  * reverb_peak_kernel       one workgroup per utterance: p, [s, e); clears the status and the clipped count.
//  * reverb_conv_kernel       direct form.  One workgroup of 256 threads owns kTile = 2048 consecutive outputs of one utterance;
//                             thread t keeps the outputs 8t .. 8t + 7 of the tile in registers, twice: all taps, and the taps
//                             inside [s, e).  The taps are walked in chunks of kChunk = 256 with the chunk of h (and its copy
//                             masked to the window) and the x window of the chunk (kTile + kChunk samples, zero outside
//                             [0, N)) in LDS as float.  Inside a chunk a step covers 8 taps: the 15 x values a thread needs
//                             are two aligned groups of 8, of which one was read by the step before, so a step costs two
//                             16-byte LDS reads of x and two of h for 64 FMAs (128 inside the window).  The LDS row of x is
//                             padded by 16 bytes every 256 so that the 32-byte lane stride does not fold onto the same banks.
//                             Every output adds its taps in ascending k with one fused multiply-add each.  Chunks whose x
//                             window lies wholly outside [0, N) are skipped (every term is an exact zero).  One pass gives
//                             y, the partial of sum e^2 and the partial of sum x^2, both in double.
//  * reverb_noise_power_kernel one workgroup per additive signal: P_j (modulo read, thread-strided, fixed tree).
//  * reverb_gains_kernel      one wave per utterance: the partials in ascending tile order -> P_before, E, then g_j.
//  * reverb_mix_kernel        the tiles again: y += g_j v_j in order j, one fused multiply-add each with g_j rounded to float,
//                             and the partial of sum y^2.
//  * reverb_scale_kernel      one wave per utterance: P_after, scale.
//  * reverb_emit_kernel       tiles of kTile outputs: shift, modulo, scale (one float product), trunc, saturate, count (an
//                             integer atomic per workgroup: exact whatever the order), to int16 and / or float32.  An
//                             utterance with a status other than 0 gets zeros.
//
// Error of the float32 output against the rule in exact arithmetic, u = 2^-24.  h and x are exact in float32.  An output of
// the convolution is L fused multiply-adds, each one rounding: |y_conv - exact| <= gamma_L A_c[n], A_c[n] = sum_k |h_k||x_{n-k}|,
// gamma_L = L u / (1 - L u), in any order of the taps.  Signal j adds one rounding of the running sum (<= u A[n], A[n] = A_c[n]
// + sum_j |g_j v_j|) and carries the relative error of its gain: one rounding of g_j to float (u), the double arithmetic behind
// it (sqrt, pow, two divisions, the sums: < 4u by a wide margin) and eta_E, the error of sqrt(E) that comes from e[n] being
// computed in float32.  |de[n]| <= gamma_W A_e[n] with W = e - s taps, so |d sum e^2| <= 2 ||e|| ||de|| and
// eta_E <= W u ||A_e||_2 / ||e||_2 to first order.  Together
//     eps[n] = (L + J + 12) u A[n] + eta_E sum_j |g_j v_j[n]|,
// where the 12 covers the gains' own roundings (5u of sum_j |g_j v_j| <= 5u A) and the second-order part of gamma_L,
// 2 L^2 u^2 A, which stays below u A for L <= 2896 (the tests use L <= 2 kChunk + 3; for a longer response read L (1 + 2 L u)
// for L); the rest is slack.  The scale is sqrt(P_before / P_after): P_before is exact (a sum of integers below 2^53),
// sqrt(sum y^2) moves by at most ||eps||_2, and the product with float(scale) rounds twice, so the relative error of the
// scaled output is delta = ||eps||_2 / ||y||_2 + 8u, and
//     |out - ref| <= scale eps[n] + |ref| delta.
// With J = 0 this is (L + J + 12) u A[n]; with additive signals the eta_E term joins it, because an early energy summed from
// float32 values cannot be bounded by a fixed number of u when e cancels.
#include <cstdio>
#include <vector>

#include "xv_kernels.h"

namespace xv {

namespace {

constexpr int kTile = XV_REVERB_TILE;      // outputs per workgroup
constexpr int kChunk = XV_REVERB_CHUNK;    // taps per LDS chunk
constexpr int kThreads = 256;
constexpr int kPer = kTile / kThreads;     // 8 consecutive outputs per thread
constexpr int kWin = kTile + kChunk;       // x window of one chunk
constexpr int kWinPad = kWin + (kWin >> 6) * 4;
static_assert(kPer == 8 && kChunk % 8 == 0 && kWin % 64 == 0, "the step of the convolution kernel is 8 taps x 8 outputs");

struct RvUtt {
  int64_t wave_off, rir_off, y_off, out_off;
  double volume;
  int32_t n, l, has_rir, before, after, y, n_out, noise_begin, noise_count, shift_output, normalize, tile_begin, tiles, pad_;
};

struct RvNoise {
  int64_t off, start;        // o_j, clamped to 2^31 - 1
  double snr;
  int32_t m, mext;
};

struct RvTile {
  int32_t utt, tile;
};

// one double per workgroup: lanes by the shuffle tree, then the four waves in order; valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ int xs_index(int i) { return i + ((i >> 6) << 2); }

__global__ __launch_bounds__(kThreads) void reverb_peak_kernel(const RvUtt* __restrict__ utts, const int16_t* __restrict__ rirs,
                                                               int32_t* __restrict__ info, int32_t* __restrict__ status,
                                                               int32_t* __restrict__ peak, int32_t* __restrict__ clipped) {
  __shared__ int best_v[kThreads / 64], best_i[kThreads / 64];
  const RvUtt u = utts[blockIdx.x];
  const int tid = threadIdx.x;
  int bv = -65536, bi = 0x7fffffff;
  if (u.has_rir) {
    const int16_t* h = rirs + u.rir_off;
    for (int k = tid; k < u.l; k += kThreads) {         // ascending k per thread: the first of equal values stays
      const int v = h[k];
      if (v > bv) { bv = v; bi = k; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int ov = __shfl_down(bv, o, 64), oi = __shfl_down(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  if ((tid & 63) == 0) { best_v[tid >> 6] = bv; best_i[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kThreads / 64; ++w)
      if (best_v[w] > bv || (best_v[w] == bv && best_i[w] < bi)) { bv = best_v[w]; bi = best_i[w]; }
    const int p = u.has_rir ? bi : 0;
    const int s = p - u.before > 0 ? p - u.before : 0;
    const int e = p + u.after < u.l ? p + u.after : u.l;
    info[blockIdx.x * 4 + 0] = p;
    info[blockIdx.x * 4 + 1] = s;
    info[blockIdx.x * 4 + 2] = e;
    info[blockIdx.x * 4 + 3] = 0;
    status[blockIdx.x] = 0;
    peak[blockIdx.x] = p;
    clipped[blockIdx.x] = 0;
  }
}

// acc[r] += sum_q hv[q] * x[r - q], x[d] = hi[d] for d >= 0 and lo[8 + d] below: taps in ascending order
__device__ __forceinline__ void step8(float (&acc)[kPer], const float (&hv)[8], const float (&lo)[8], const float (&hi)[8]) {
#pragma unroll
  for (int q = 0; q < 8; ++q)
#pragma unroll
    for (int r = 0; r < kPer; ++r) acc[r] = fmaf(hv[q], r - q >= 0 ? hi[r - q] : lo[8 + r - q], acc[r]);
}

__device__ __forceinline__ void load8(float (&d)[8], const float* p) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w;
  d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
}

__global__ __launch_bounds__(kThreads) void reverb_conv_kernel(const RvUtt* __restrict__ utts, const RvTile* __restrict__ tiles,
                                                               const int16_t* __restrict__ waves, const int16_t* __restrict__ rirs,
                                                               const int32_t* __restrict__ info, float* __restrict__ ybuf,
                                                               double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float xs[kWinPad];
  __shared__ __attribute__((aligned(16))) float hs[kChunk];
  __shared__ __attribute__((aligned(16))) float he[kChunk];
  __shared__ double red[kThreads / 64];
  const RvTile tl = tiles[blockIdx.x];
  const RvUtt u = utts[tl.utt];
  const int tid = threadIdx.x;
  const int64_t n0 = (int64_t)tl.tile * kTile;
  const int ws = info[tl.utt * 4 + 1], we = info[tl.utt * 4 + 2];
  const int16_t* x = waves + u.wave_off;
  const int16_t* h = rirs + u.rir_off;            // not read without an RIR

  float acc[kPer], eacc[kPer];
#pragma unroll
  for (int r = 0; r < kPer; ++r) acc[r] = eacc[r] = 0.f;

  // chunk c reads x[n0 - cC - C .. n0 - cC + T): only the chunks whose window meets [0, N) can add anything
  const int nchunks = (u.l + kChunk - 1) / kChunk;
  int64_t c_lo = (n0 - u.n) / kChunk;                // first c with n0 - cC - C < N  <=>  c > (n0 - N) / C - 1
  if (n0 - u.n < 0) c_lo = 0;
  int64_t c_hi = (n0 + kTile - 1) / kChunk;          // last c with n0 - cC + T - 1 >= 0
  if (c_hi > nchunks - 1) c_hi = nchunks - 1;
  for (int64_t c = c_lo; c <= c_hi; ++c) {
    const int k0 = (int)c * kChunk;
    const int64_t g0 = n0 - k0 - kChunk;
    __syncthreads();                                 // the chunk before has been consumed
    for (int j = tid; j < kWin; j += kThreads) {
      const int64_t g = g0 + j;
      xs[xs_index(j)] = g >= 0 && g < u.n ? (float)x[g] : 0.f;
    }
    {
      const int k = k0 + tid;                        // kChunk == kThreads
      float v = 0.f;
      if (k < u.l) v = u.has_rir ? (float)h[k] * (1.0f / 32768.0f) : 1.0f;
      hs[tid] = v;
      he[tid] = k >= ws && k < we ? v : 0.f;
    }
    __syncthreads();
    const bool chunk_early = k0 < we && k0 + kChunk > ws;
    float hi[8], lo[8], hv[8];
    int g = kChunk / 8 + tid;                        // group of 8 floats holding x[n - k0], n = the thread's first output
    load8(hi, xs + xs_index(8 * g));
#pragma unroll 2
    for (int s = 0; s < kChunk / 8; ++s) {
      --g;
      load8(lo, xs + xs_index(8 * g));
      load8(hv, hs + 8 * s);
      step8(acc, hv, lo, hi);
      if (chunk_early && k0 + 8 * s < we && k0 + 8 * s + 8 > ws) {       // uniform over the workgroup
        load8(hv, he + 8 * s);
        step8(eacc, hv, lo, hi);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) hi[i] = lo[i];
    }
  }

  double se = 0.0, sx = 0.0;
  const int64_t n = n0 + (int64_t)tid * kPer;
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    if (n + r < u.y) {
      ybuf[u.y_off + n + r] = acc[r];
      se += (double)eacc[r] * (double)eacc[r];
    }
    if (n + r < u.n) {
      const double v = (double)x[n + r];
      sx += v * v;
    }
  }
  se = block_sum(se, red);
  sx = block_sum(sx, red);
  if (tid == 0) {
    double* p = part + (int64_t)(u.tile_begin + tl.tile) * 3;
    p[0] = sx;
    p[1] = se;
  }
}

__global__ __launch_bounds__(kThreads) void reverb_noise_power_kernel(const RvNoise* __restrict__ noises,
                                                                      const int16_t* __restrict__ sig, double* __restrict__ nd) {
  __shared__ double red[kThreads / 64];
  const RvNoise nz = noises[blockIdx.x];
  const int16_t* v = sig + nz.off;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < nz.mext; i += kThreads) {
    const double a = (double)v[(uint32_t)i % (uint32_t)nz.m];
    s += a * a;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) nd[blockIdx.x * 2] = s / (double)nz.mext;
}

// lane l adds the partials l, l + 64, ... of the utterance's tiles in ascending order, then the shuffle tree
__device__ __forceinline__ double tile_sum(const double* part, int tile_begin, int tiles, int k, int lane) {
  double v = 0.0;
  for (int t = lane; t < tiles; t += 64) v += part[(int64_t)(tile_begin + t) * 3 + k];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return __shfl(v, 0, 64);
}

__global__ __launch_bounds__(64) void reverb_gains_kernel(const RvUtt* __restrict__ utts, const RvNoise* __restrict__ noises,
                                                          const int32_t* __restrict__ info, const double* __restrict__ part,
                                                          double* __restrict__ ud, double* __restrict__ nd,
                                                          int32_t* __restrict__ status) {
  const RvUtt u = utts[blockIdx.x];
  const int lane = threadIdx.x;
  const double sx = tile_sum(part, u.tile_begin, u.tiles, 0, lane);
  const double se = tile_sum(part, u.tile_begin, u.tiles, 1, lane);
  const int ws = info[blockIdx.x * 4 + 1], we = info[blockIdx.x * 4 + 2];
  const double p_before = sx / (double)u.n;
  const double early = se / (double)((int64_t)u.n + (we - ws) - 1);
  if (lane == 0) {
    ud[blockIdx.x * 4 + 0] = p_before;
    ud[blockIdx.x * 4 + 1] = early;
  }
  for (int j = lane; j < u.noise_count; j += 64) {
    const int64_t row = (int64_t)u.noise_begin + j;
    const double p = nd[row * 2];
    double g = 0.0;
    if (p > 0.0) g = sqrt(pow(10.0, -noises[row].snr / 10.0) * early / p);
    else status[blockIdx.x] = 1;                     // every lane that gets here writes the same value
    nd[row * 2 + 1] = g;
  }
}

__global__ __launch_bounds__(kThreads) void reverb_mix_kernel(const RvUtt* __restrict__ utts, const RvTile* __restrict__ tiles,
                                                              const RvNoise* __restrict__ noises, const int16_t* __restrict__ sig,
                                                              const double* __restrict__ nd, const int32_t* __restrict__ status,
                                                              float* __restrict__ ybuf, double* __restrict__ part) {
  __shared__ double red[kThreads / 64];
  const RvTile tl = tiles[blockIdx.x];
  const RvUtt u = utts[tl.utt];
  const int64_t n0 = (int64_t)tl.tile * kTile;
  const bool mix = u.noise_count > 0 && status[tl.utt] == 0;
  float* y = ybuf + u.y_off;
  double sy = 0.0;
  for (int i = 0; i < kPer; ++i) {
    const int64_t n = n0 + i * kThreads + threadIdx.x;
    if (n >= u.y) break;
    float v = y[n];
    if (mix) {
      for (int j = 0; j < u.noise_count; ++j) {
        const RvNoise nz = noises[u.noise_begin + j];
        const int64_t k = n - nz.start;
        if (k >= 0 && k < nz.mext) v = fmaf((float)nd[(int64_t)(u.noise_begin + j) * 2 + 1], (float)sig[nz.off + (uint32_t)k % (uint32_t)nz.m], v);
      }
      y[n] = v;
    }
    sy += (double)v * (double)v;
  }
  sy = block_sum(sy, red);
  if (threadIdx.x == 0) part[(int64_t)(u.tile_begin + tl.tile) * 3 + 2] = sy;
}

__global__ __launch_bounds__(64) void reverb_scale_kernel(const RvUtt* __restrict__ utts, const double* __restrict__ part,
                                                          double* __restrict__ ud, int32_t* __restrict__ status) {
  const RvUtt u = utts[blockIdx.x];
  const double sy = tile_sum(part, u.tile_begin, u.tiles, 2, threadIdx.x);
  if (threadIdx.x != 0) return;
  const double p_after = sy / (double)u.y;
  double scale = 1.0;
  if (u.volume > 0.0) {
    scale = u.volume;
  } else if (u.normalize) {
    if (p_after > 0.0) {
      scale = sqrt(ud[blockIdx.x * 4 + 0] / p_after);
    } else {
      scale = 0.0;
      if (status[blockIdx.x] == 0) status[blockIdx.x] = 2;
    }
  }
  ud[blockIdx.x * 4 + 2] = p_after;
  ud[blockIdx.x * 4 + 3] = scale;
}

__global__ __launch_bounds__(kThreads) void reverb_emit_kernel(const RvUtt* __restrict__ utts, const RvTile* __restrict__ tiles,
                                                               const int32_t* __restrict__ info, const double* __restrict__ ud,
                                                               const int32_t* __restrict__ status, const float* __restrict__ ybuf,
                                                               int16_t* __restrict__ out16, float* __restrict__ out32,
                                                               int32_t* __restrict__ clipped) {
  __shared__ int red[kThreads / 64];
  const RvTile tl = tiles[blockIdx.x];
  const RvUtt u = utts[tl.utt];
  const int64_t i0 = (int64_t)tl.tile * kTile;
  const bool ok = status[tl.utt] == 0;
  const float scale = (float)ud[tl.utt * 4 + 3];
  const int64_t shift = u.has_rir && u.shift_output ? info[tl.utt * 4 + 0] : 0;
  const float* y = ybuf + u.y_off;
  int cnt = 0;
  for (int r = 0; r < kPer; ++r) {
    const int64_t i = i0 + r * kThreads + threadIdx.x;
    if (i >= u.n_out) break;
    const float v = ok ? scale * y[(uint32_t)(i + shift) % (uint32_t)u.y] : 0.f;
    if (out32) out32[u.out_off + i] = v;
    if (out16) {
      float t = truncf(v);
      if (t > 32767.f) { t = 32767.f; ++cnt; }
      if (t < -32768.f) { t = -32768.f; ++cnt; }
      out16[u.out_off + i] = (int16_t)(int)t;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int total = red[0] + red[1] + red[2] + red[3];
    if (total > 0) atomicAdd(&clipped[tl.utt], total);
  }
}

int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

struct Layout {
  int64_t conv_tiles = 0, emit_tiles = 0, y_floats = 0;
  int64_t off_utts, off_noises, off_ctiles, off_etiles, table_bytes;      // the host-built block, copied in one piece
  int64_t off_info, off_part, off_ud, off_nd, off_y, total;
};

Layout layout_of(const xv_reverb_utt* utts, int64_t nu, int64_t nn) {
  Layout l;
  for (int64_t i = 0; i < nu; ++i) {
    const int64_t L = utts[i].rir_len > 0 ? utts[i].rir_len : 1;
    const int64_t y = utts[i].wave_len + L - 1;
    l.conv_tiles += (y + kTile - 1) / kTile;
    l.emit_tiles += (utts[i].out_len + kTile - 1) / kTile;
    l.y_floats += (y + 63) / 64 * 64;
  }
  l.off_utts = 0;
  l.off_noises = align256(nu * (int64_t)sizeof(RvUtt));
  l.off_ctiles = l.off_noises + align256(nn * (int64_t)sizeof(RvNoise));
  l.off_etiles = l.off_ctiles + align256(l.conv_tiles * (int64_t)sizeof(RvTile));
  l.table_bytes = l.off_etiles + align256(l.emit_tiles * (int64_t)sizeof(RvTile));
  l.off_info = l.table_bytes;
  l.off_part = l.off_info + align256(nu * 16);
  l.off_ud = l.off_part + align256(l.conv_tiles * 24);
  l.off_nd = l.off_ud + align256(nu * 32);
  l.off_y = l.off_nd + align256(nn * 16);
  l.total = l.off_y + align256(l.y_floats * 4);
  return l;
}

void free_table(void* p) { delete static_cast<std::vector<char>*>(p); }

}  // namespace

int64_t reverb_out_len(const xv_reverb_utt& u) {
  if (u.duration > 0.0) return (int64_t)(u.duration * u.sample_rate);
  if (u.shift_output) return u.wave_len;
  return u.wave_len + (u.rir_len > 0 ? u.rir_len : 1) - 1;
}

int reverb_validate(const xv_reverb_utt* utts, int64_t nu, const xv_reverb_noise* noises, int64_t nn, int64_t wave_samples,
                    int64_t rir_samples, int64_t noise_samples, int64_t out_samples, std::string* err) {
  const int64_t lim = (int64_t)1 << 31;
  char buf[200];
  auto bad = [&](int code, int64_t i, const char* what) {
    snprintf(buf, sizeof(buf), "utterance %lld: %s", (long long)i, what);
    *err = buf;
    return code;
  };
  if (nu < 1 || nu >= lim || nn < 0 || nn >= lim || !utts || (nn > 0 && !noises) || wave_samples < 0 || rir_samples < 0 ||
      noise_samples < 0 || out_samples < 0) {
    *err = "bad table sizes (num_utts >= 1, num_noises >= 0, sample counts >= 0)";
    return XV_ERR_INVALID;
  }
  int64_t wave_end = 0, out_end = 0, noise_end = 0, tiles = 0;
  for (int64_t i = 0; i < nu; ++i) {
    const xv_reverb_utt& u = utts[i];
    if (u.wave_len < 1 || u.wave_len >= lim) return bad(XV_ERR_INVALID, i, "wave_len outside [1, 2^31)");
    if (u.wave_off < wave_end || u.wave_off > wave_samples - u.wave_len) return bad(XV_ERR_INVALID, i, "wave offsets must rise and stay inside the buffer");
    wave_end = u.wave_off + u.wave_len;
    if (u.rir_len < 0) return bad(XV_ERR_INVALID, i, "negative rir_len");
    if (u.rir_len > XV_REVERB_MAX_TAPS) return bad(XV_ERR_UNSUPPORTED, i, "an impulse response of more than 65536 taps");
    if (u.rir_len > 0 && (u.rir_off < 0 || u.rir_off > rir_samples - u.rir_len)) return bad(XV_ERR_INVALID, i, "the impulse response lies outside the buffer");
    if (!(u.sample_rate >= 100.0 && u.sample_rate <= 1e6)) return bad(XV_ERR_INVALID, i, "sample_rate outside [100, 1e6]");
    if (!(u.duration >= 0.0) || !(u.duration < 1e9) || !(u.volume >= 0.0) || !(u.volume <= 1e6)) return bad(XV_ERR_INVALID, i, "duration / volume must be finite and not negative (volume <= 1e6)");
    const int64_t y = u.wave_len + (u.rir_len > 0 ? u.rir_len : 1) - 1;
    if (y >= lim) return bad(XV_ERR_INVALID, i, "N + L - 1 reaches 2^31");
    const int64_t n_out = reverb_out_len(u);
    if (n_out >= lim) return bad(XV_ERR_INVALID, i, "the output length reaches 2^31");
    if (u.out_len != n_out) return bad(XV_ERR_INVALID, i, "out_len differs from the rule's n_out");
    if (u.out_off < out_end || u.out_off > out_samples - u.out_len) return bad(XV_ERR_INVALID, i, "output offsets must rise and stay inside the buffer");
    out_end = u.out_off + u.out_len;
    if (u.noise_count < 0 || u.noise_begin < noise_end || u.noise_begin > nn - u.noise_count) return bad(XV_ERR_INVALID, i, "noise rows must rise and stay inside the table");
    noise_end = u.noise_begin + u.noise_count;
    for (int64_t j = u.noise_begin; j < noise_end; ++j) {
      const xv_reverb_noise& z = noises[j];
      if (z.len < 1 || z.len >= lim || z.ext_len < 1 || z.ext_len >= lim) return bad(XV_ERR_INVALID, i, "an additive signal's len / ext_len outside [1, 2^31)");
      if (z.off < 0 || z.off > noise_samples - z.len) return bad(XV_ERR_INVALID, i, "an additive signal lies outside the buffer");
      if (!(z.snr_db >= -200.0 && z.snr_db <= 200.0)) return bad(XV_ERR_INVALID, i, "an snr outside [-200, 200] dB");
      if (!(z.start_time >= 0.0) || !(z.start_time < 1e9)) return bad(XV_ERR_INVALID, i, "a start time that is negative or not finite");
    }
    tiles += (y + kTile - 1) / kTile + (n_out + kTile - 1) / kTile;
    if (tiles >= lim) return bad(XV_ERR_INVALID, i, "the batch has 2^31 tiles or more: split it");
  }
  return XV_OK;
}

int64_t reverb_workspace_bytes(const xv_reverb_utt* utts, int64_t nu, int64_t nn) { return layout_of(utts, nu, nn).total; }

hipError_t launch_reverb(const int16_t* waves, const int16_t* rirs, const int16_t* sig, const xv_reverb_utt* utts, int64_t nu,
                         const xv_reverb_noise* noises, int64_t nn, int16_t* out16, float* out32, int32_t* status, int32_t* peak,
                         int32_t* clipped, void* ws, hipStream_t stream) {
  const Layout l = layout_of(utts, nu, nn);
  auto* table = new std::vector<char>((size_t)l.table_bytes, 0);
  RvUtt* du = reinterpret_cast<RvUtt*>(table->data() + l.off_utts);
  RvNoise* dn = reinterpret_cast<RvNoise*>(table->data() + l.off_noises);
  RvTile* ct = reinterpret_cast<RvTile*>(table->data() + l.off_ctiles);
  RvTile* et = reinterpret_cast<RvTile*>(table->data() + l.off_etiles);
  int64_t y_off = 0, nc = 0, ne = 0;
  for (int64_t i = 0; i < nu; ++i) {
    const xv_reverb_utt& u = utts[i];
    RvUtt& d = du[i];
    d.wave_off = u.wave_off;
    d.rir_off = u.rir_len > 0 ? u.rir_off : 0;
    d.y_off = y_off;
    d.out_off = u.out_off;
    d.volume = u.volume;
    d.n = (int32_t)u.wave_len;
    d.has_rir = u.rir_len > 0;
    d.l = d.has_rir ? (int32_t)u.rir_len : 1;
    d.before = (int32_t)(0.001 * u.sample_rate);
    d.after = (int32_t)(0.05 * u.sample_rate);
    d.y = d.n + d.l - 1;
    d.n_out = (int32_t)u.out_len;
    d.noise_begin = (int32_t)u.noise_begin;
    d.noise_count = (int32_t)u.noise_count;
    d.shift_output = u.shift_output != 0;
    d.normalize = u.normalize_output != 0;
    d.tile_begin = (int32_t)nc;
    d.tiles = (d.y + kTile - 1) / kTile;
    for (int t = 0; t < d.tiles; ++t) ct[nc++] = RvTile{(int32_t)i, t};
    for (int t = 0; t < (d.n_out + kTile - 1) / kTile; ++t) et[ne++] = RvTile{(int32_t)i, t};
    y_off += ((int64_t)d.y + 63) / 64 * 64;
    for (int64_t j = u.noise_begin; j < u.noise_begin + u.noise_count; ++j) {
      const xv_reverb_noise& z = noises[j];
      const double o = z.start_time * u.sample_rate;
      dn[j] = RvNoise{z.off, o < 2147483647.0 ? (int64_t)o : (int64_t)2147483647, z.snr_db, (int32_t)z.len, (int32_t)z.ext_len};
    }
  }
  char* w = static_cast<char*>(ws);
  hipError_t e = hipMemcpyAsync(w, table->data(), (size_t)l.table_bytes, hipMemcpyHostToDevice, stream);
  // the copy may still be reading the table when this returns: it is freed in stream order, behind the copy
  if (hipLaunchHostFunc(stream, free_table, table) != hipSuccess) {
    (void)hipStreamSynchronize(stream);
    delete table;
  }
  if (e != hipSuccess) return e;
  const RvUtt* gu = reinterpret_cast<const RvUtt*>(w + l.off_utts);
  const RvNoise* gn = reinterpret_cast<const RvNoise*>(w + l.off_noises);
  const RvTile* gct = reinterpret_cast<const RvTile*>(w + l.off_ctiles);
  const RvTile* get = reinterpret_cast<const RvTile*>(w + l.off_etiles);
  int32_t* info = reinterpret_cast<int32_t*>(w + l.off_info);
  double* part = reinterpret_cast<double*>(w + l.off_part);
  double* ud = reinterpret_cast<double*>(w + l.off_ud);
  double* nd = reinterpret_cast<double*>(w + l.off_nd);
  float* ybuf = reinterpret_cast<float*>(w + l.off_y);
  hipLaunchKernelGGL(reverb_peak_kernel, dim3((unsigned)nu), dim3(kThreads), 0, stream, gu, rirs, info, status, peak, clipped);
  hipLaunchKernelGGL(reverb_conv_kernel, dim3((unsigned)l.conv_tiles), dim3(kThreads), 0, stream, gu, gct, waves, rirs, info, ybuf,
                     part);
  if (nn > 0) hipLaunchKernelGGL(reverb_noise_power_kernel, dim3((unsigned)nn), dim3(kThreads), 0, stream, gn, sig, nd);
  hipLaunchKernelGGL(reverb_gains_kernel, dim3((unsigned)nu), dim3(64), 0, stream, gu, gn, info, part, ud, nd, status);
  hipLaunchKernelGGL(reverb_mix_kernel, dim3((unsigned)l.conv_tiles), dim3(kThreads), 0, stream, gu, gct, gn, sig, nd, status, ybuf,
                     part);
  hipLaunchKernelGGL(reverb_scale_kernel, dim3((unsigned)nu), dim3(64), 0, stream, gu, part, ud, status);
  if (l.emit_tiles > 0)
    hipLaunchKernelGGL(reverb_emit_kernel, dim3((unsigned)l.emit_tiles), dim3(kThreads), 0, stream, gu, get, info, ud, status, ybuf,
                       out16, out32, clipped);
  return hipGetLastError();
}

}  // namespace xv
