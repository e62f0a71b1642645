// Forward and backward of one frame-level layer on packed utterances: a W-tap temporal convolution (VALID, stride 1, no
// dilation: tf.layers.conv2d(.., (1, W)) / tf.layers.conv1d(.., W) of model/tdnn.py) + batch norm (inference mode) + activation,
// with the CURRENT weights.  With W = 1 it is the dense layer of csrc/seg_grad.hip.  The rule is stated in include/xvec_hip.h
// (xv_tconv_forward, xv_tconv_backward) and restated in float64 numpy in tests/helpers/ref_tconv.py; torch.autograd of conv1d +
// eval-mode batch_norm + relu / leaky_relu(0.2) gives the same numbers (tests/test_tconv_host.py).
//
// Nothing is unfolded and nothing is scattered.  Output row t of an utterance reads the W consecutive input rows t .. t + W - 1,
// so row t of the im2col matrix [total_out, K = W C] is a VIEW of x: element k = tau C + c lives at (row + tau) ldx + c.  All
// three products are exact-fp32 GEMMs on v_mfma_f32_32x32x2_f32 over such views, 64 x 64 tiles, a reduction step of 32,
// zero-filled edges, register-staged double buffering (the K-step body of csrc/nt_gemm.h with two kinds of operand tile: rows
// along the reduction, read from LDS as one 16-byte word, and the reduction along the rows, read as four words):
//  * tc_scan_kernel, tc_map_kernel: out_off[b] = sum_{a < b} max(n_in_a - (W - 1), 0) on the device, then for every output row
//    its first input row, and for every owned input row (its index in its utterance, out_off, n_out, its absolute row).
//  * tc_gemm_kernel<TC_FWD>: z = im2col(x) . w^T + b, then h and y in the epilogue by the lines of csrc/layer_lines.h (bn_r,
//    bn_h, act_y).  The chain of z runs over k ascending from 0, a function of W C alone; the bias comes last.
//  * tc_mask_kernel: a = gy act'(h) by act_grad (h from the stored z by bn_h, the forward's), gz = a s_j, written once as gz
//    [total_out, round4(N)].  The rows are cut into R slices of `rows_per_slice` rows (tc_slices: a function of total_out alone);
//    within a slice lane l of the wave that owns column j adds the rows i = l (mod 64) in ascending order to three doubles (a,
//    a r (z - mm), gz), a fixed xor butterfly over the 64 lanes closes the slice; tc_colsum_kernel adds the R slice sums in
//    ascending order in double and rounds once.
//  * tc_gemm_kernel<TC_GW>: gw = gz^T . im2col(x), both operands read along the reduction (the output rows).  The chain of one
//    element runs over the output rows ascending.  Where the tiles alone would not fill the device (the first layer: K = 150),
//    the rows are cut into S contiguous ranges (tc_split: a function of N, K and total_out alone), every range sums into its own
//    plane of the workspace from zero, and tc_gwsum_kernel adds the S planes in ascending order, float32, one rounding each.
//  * tc_gemm_kernel<TC_GX>: gx [input rows, C] = G . w', where row s of G is the gather [gz_b[s - 0], gz_b[s - 1], ..,
//    gz_b[s - (W - 1)]] (zeros where s - tau falls outside the utterance's output rows) and w'[tau round4(N) + j][c] =
//    w[j][tau C + c], read in place.  One writer per element of gx: a gather, not a col2im scatter.  The chain runs over tau
//    ascending, then j ascending; the round4(N) - N padding columns multiply exact zeros.
// Every element of every output is a function of the inputs alone: one writer per element, a fixed order, no floating-point
// atomics, no value read from memory this call did not write.  z, y and gx of an utterance use its own rows and the parameters
// only, and the order of their chains does not depend on where the utterance lies.  Nothing of the workspace depends on
// ws_bytes: xv_tconv_workspace_min and xv_tconv_workspace agree, and a larger workspace is not used.
//
// Error bound (u = 2^-24; checked per element in tests/test_gpu_tconv.py, restated in ref_tconv.bounds).  |.| of the float64
// oracle's values; n = total output rows, X = the im2col view of x, K = W C; t = 2^-53 (n + 64) covers the double sums:
//   z_ij:      Bz = (K + 2) u (sum_k |X_ik w_jk| + |b_j|)                     (fmaf chain of length K, then the bias)
//   h, y, a, gz, gbeta, ggamma, gbias: the bounds of csrc/layer_lines.h with this Bz
//   gw_jk:     sum_i Bg |X_ik| + (n + 64) u sum_i |gz_ij X_ik|               (S chains of at most n / S + 32 steps, padded to 32,
//              then S - 1 <= 31 additions)
//   gx_sc:     sum_{tau, j} Bg |w_j,tau C + c| + (W (N + 3) + 2) u sum_{tau, j} |gz_{s - tau, j} w_j,tau C + c|
#include "layer_lines.h"
#include "nt_gemm.h"

namespace xv {

using ntg::gf32x16;
using ntg::gf32x4;
using ntg::up;

namespace {

constexpr int kTcTile = 64;
constexpr int kTcBK = 32;
constexpr int kTcLdRow = kTcBK + 4;           // operand tile [64 rows][32 k + 4]
constexpr int kTcLdRed = kTcTile + 8;         // operand tile [32 k][64 rows + 8]
constexpr int kTcTileFloats = kTcTile * kTcLdRow;
static_assert(kTcBK * kTcLdRed == kTcTileFloats, "both tile kinds take the same LDS");
constexpr int kTcMaxSplit = 32;
constexpr int kTcMaxSlices = 64;

enum { TC_FWD = 0, TC_GW = 1, TC_GX = 2 };

// ---------------------------------------------------------------------------------------------- offsets and row maps
// out_off [batch + 1]: one workgroup walks the utterances in chunks of 256 with a running carry
__global__ __launch_bounds__(256) void tc_scan_kernel(const int32_t* __restrict__ in_off, int64_t batch, int W, int32_t* __restrict__ out_off) {
  __shared__ int sums[256];
  __shared__ int carry;
  const int tid = threadIdx.x;
  if (tid == 0) {
    carry = 0;
    out_off[0] = 0;
  }
  __syncthreads();
  for (int64_t b0 = 0; b0 < batch; b0 += 256) {
    const int64_t b = b0 + tid;
    int v = 0;
    if (b < batch) {
      v = in_off[b + 1] - in_off[b] - (W - 1);
      if (v < 0) v = 0;
    }
    sums[tid] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const int add = tid >= o ? sums[tid - o] : 0;
      __syncthreads();
      sums[tid] += add;
      __syncthreads();
    }
    if (b < batch) out_off[b + 1] = carry + sums[tid];
    __syncthreads();
    if (tid == 255) carry += sums[255];
    __syncthreads();
  }
}

// the utterance that owns position v of an ascending offsets array: the last b with off[b] <= v (off[0] <= v < off[batch])
__device__ __forceinline__ int64_t tc_owner(const int32_t* off, int64_t batch, int64_t v) {
  int64_t lo = 0, hi = batch;                 // off[lo] <= v < off[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid] <= v) lo = mid; else hi = mid;
  }
  return lo;
}

// rowmap [total_out]: the first input row of output row r, -1 beyond the last output row.
// info [total_in]: for input row in_off[0] + i: (index in its utterance, out_off of the utterance, its n_out, the absolute row);
// index -1 beyond the last owned row.
__global__ __launch_bounds__(256) void tc_map_kernel(const int32_t* __restrict__ in_off, const int32_t* __restrict__ out_off,
                                                     int64_t batch, int64_t total_out, int64_t total_in, int32_t* __restrict__ rowmap,
                                                     int4* __restrict__ info) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < total_out) {
    int32_t v = -1;
    if (i < out_off[batch]) {
      const int64_t b = tc_owner(out_off, batch, i);
      v = in_off[b] + (int32_t)(i - out_off[b]);
    }
    rowmap[i] = v;
  }
  if (info && i < total_in) {
    int4 v = make_int4(-1, 0, 0, 0);
    const int64_t s = (int64_t)in_off[0] + i;
    if (s < in_off[batch]) {
      const int64_t b = tc_owner(in_off, batch, s);
      v = make_int4((int)(s - in_off[b]), out_off[b], out_off[b + 1] - out_off[b], (int)s);
    }
    info[i] = v;
  }
}

// ---------------------------------------------------------------------------------------------- the three products
struct TcGemmArgs {
  const float* x; int64_t ldx; int C, W;      // the packed input, K = W C
  const float* w; int64_t ldw; int N;         // [N, ldw], K columns
  const int32_t* rowmap; int64_t total_out;
  const int4* info; int64_t total_in;
  const float* gz; int64_t ldg;               // [total_out, ldg]
  int nMt, nNt;
  // TC_FWD
  const float *bias, *gamma, *beta, *mm, *mv;
  int act;
  float* z; int64_t ldz; float* y; int64_t ldy;
  // TC_GW: split s takes the output rows [s rows_per_split, (s + 1) rows_per_split); out = gw, or the planes when split > 1
  int split; int64_t rows_per_split;
  // TC_GW, TC_GX
  float* out; int64_t ldo;
};

// four consecutive elements k .. k + 3 of the im2col row that starts at input row `row` (k < K, a multiple of 4)
template <bool VEC>
__device__ __forceinline__ gf32x4 tc_load_x(const float* __restrict__ x, int64_t ldx, int C, int K, int64_t row, int k) {
  gf32x4 v = {0.f, 0.f, 0.f, 0.f};
  int tau = k / C, c = k - tau * C;
  if (VEC) return *reinterpret_cast<const gf32x4*>(x + (row + tau) * ldx + c);     // C % 4 == 0: one tap, 16-byte aligned
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (k + e < K) v[e] = x[(row + tau) * ldx + c];
    if (++c == C) { c = 0; ++tau; }
  }
  return v;
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(256, 2) void tc_gemm_kernel(TcGemmArgs p) {
  // A and B, two buffers each.  Tile kinds: TC_FWD A rows, B rows; TC_GW A red, B red; TC_GX A rows, B red.
  __shared__ __attribute__((aligned(16))) float smem[4 * kTcTileFloats];
  constexpr bool A_RED = MODE == TC_GW, B_RED = MODE != TC_FWD;
  float* As = smem;
  float* Bs = smem + 2 * kTcTileFloats;
  const int mt = (int)(blockIdx.x % (unsigned)p.nMt), nt = (int)(blockIdx.x / (unsigned)p.nMt);
  const ntg::NtPos<64, 64> at(mt, nt);
  const int tid = threadIdx.x;
  const int K = p.W * p.C;

  // staging coordinates: a rows tile takes (row lr + 32 i, k 4 c4), a red tile (k kr + 16 i, row 4 c16)
  const int c4 = tid & 7, lr = tid >> 3;
  const int c16 = tid & 15, kr = tid >> 4;

  // the reduction: its range and what each thread keeps of its two staging rows
  int64_t red0 = 0, red1 = 0;
  int64_t arow[2] = {-1, -1};                 // TC_FWD: first input row of the output row; TC_GX: unused
  int4 ainf[2];                               // TC_GX
  if (MODE == TC_FWD) {
    red1 = K;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t r = (int64_t)at.m0 + lr + 32 * i;
      if (r < p.total_out) arow[i] = p.rowmap[r];
    }
  } else if (MODE == TC_GW) {
    red0 = (int64_t)blockIdx.y * p.rows_per_split;
    red1 = red0 + p.rows_per_split < p.total_out ? red0 + p.rows_per_split : p.total_out;
  } else {
    red1 = (int64_t)p.W * p.ldg;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t sl = (int64_t)at.m0 + lr + 32 * i;
      ainf[i] = sl < p.total_in ? p.info[sl] : make_int4(-1, 0, 0, 0);
    }
  }
  const int nk = (int)((red1 - red0 + kTcBK - 1) / kTcBK);

  gf32x4 ra[2], rb[2];
  auto load_tiles = [&](int kt) {
    const int64_t k0 = red0 + (int64_t)kt * kTcBK;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      gf32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
      if (MODE == TC_FWD) {
        const int k = (int)k0 + 4 * c4;
        if (arow[i] >= 0 && k < K) a = tc_load_x<VEC>(p.x, p.ldx, p.C, K, arow[i], k);
        const int j = at.n0 + lr + 32 * i;
        if (j < p.N && k < K) {
          const float* src = p.w + (int64_t)j * p.ldw + k;
          if (VEC) {
            b = *reinterpret_cast<const gf32x4*>(src);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (k + e < K) b[e] = src[e];
          }
        }
      } else if (MODE == TC_GW) {
        const int64_t r = k0 + kr + 16 * i;
        const int64_t xr = r < red1 ? p.rowmap[r] : -1;
        const int j = at.m0 + 4 * c16, k = at.n0 + 4 * c16;
        if (xr >= 0) {
          if (j < p.N) a = *reinterpret_cast<const gf32x4*>(p.gz + r * p.ldg + j);      // columns N .. ldg feed rows never stored
          if (k < K) b = tc_load_x<VEC>(p.x, p.ldx, p.C, K, xr, k);
        }
      } else {
        {
          const int64_t kk = k0 + 4 * c4;                        // tau ldg + j, j a multiple of 4
          const int tau = (int)(kk / p.ldg), j = (int)(kk - (int64_t)tau * p.ldg);
          const int tl = ainf[i].x - tau;
          if (kk < red1 && ainf[i].x >= 0 && tl >= 0 && tl < ainf[i].z && j < p.N) {
            a = *reinterpret_cast<const gf32x4*>(p.gz + ((int64_t)ainf[i].y + tl) * p.ldg + j);
#pragma unroll
            for (int e = 1; e < 4; ++e)
              if (j + e >= p.N) a[e] = 0.f;                       // the padding columns of gz hold nothing
          }
        }
        const int64_t kk = k0 + kr + 16 * i;
        const int tau = (int)(kk / p.ldg), j = (int)(kk - (int64_t)tau * p.ldg);
        const int c = at.n0 + 4 * c16;
        if (kk < red1 && j < p.N && c < p.C) {
          const float* src = p.w + (int64_t)j * p.ldw + (int64_t)tau * p.C + c;
          if (VEC) {
            b = *reinterpret_cast<const gf32x4*>(src);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (c + e < p.C) b[e] = src[e];
          }
        }
      }
      ra[i] = a;
      rb[i] = b;
    }
  };
  auto store_tiles = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float* da = As + buf * kTcTileFloats + (A_RED ? (kr + 16 * i) * kTcLdRed + 4 * c16 : (lr + 32 * i) * kTcLdRow + 4 * c4);
      float* db = Bs + buf * kTcTileFloats + (B_RED ? (kr + 16 * i) * kTcLdRed + 4 * c16 : (lr + 32 * i) * kTcLdRow + 4 * c4);
      *reinterpret_cast<gf32x4*>(da) = ra[i];
      *reinterpret_cast<gf32x4*>(db) = rb[i];
    }
  };

  gf32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;

  if (nk > 0) {
    load_tiles(0);
    store_tiles(0);
  }
  __syncthreads();
  const int arow_l = at.wm * 32 + at.r32, brow_l = at.wn * 32 + at.r32;
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load_tiles(kt + 1);
    const float* ap = As + cur * kTcTileFloats;
    const float* bp = Bs + cur * kTcTileFloats;
#pragma unroll
    for (int q = 0; q < kTcBK / 8; ++q) {
      // lane (r, h) feeds k = 8 q + 4 h + j of both operands: the order of the chain is a function of k alone
      gf32x4 a, b;
      if (A_RED) {
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = ap[(8 * q + 4 * at.h + j) * kTcLdRed + arow_l];
      } else {
        a = *reinterpret_cast<const gf32x4*>(ap + arow_l * kTcLdRow + 8 * q + 4 * at.h);
      }
      if (B_RED) {
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = bp[(8 * q + 4 * at.h + j) * kTcLdRed + brow_l];
      } else {
        b = *reinterpret_cast<const gf32x4*>(bp + brow_l * kTcLdRow + 8 * q + 4 * at.h);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
    }
    if (kt + 1 < nk) store_tiles(cur ^ 1);
    __syncthreads();
  }

  const int gj = at.col(0);
  if (MODE == TC_FWD) {
    if (gj >= p.N) return;
    const float bj = p.bias[gj];
    float s = 0.f, mm = 0.f, beta = 0.f;
    if (p.gamma) {
      s = __fmul_rn(p.gamma[gj], lines::bn_r(p.mv[gj]));
      mm = p.mm[gj];
      beta = p.beta[gj];
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int64_t gi = at.row(0, e);
      if (gi >= p.total_out || p.rowmap[gi] < 0) continue;
      const float z = __fadd_rn(acc[e], bj);
      const float h = p.gamma ? lines::bn_h(z, s, mm, beta) : z;
      p.z[gi * p.ldz + gj] = z;
      p.y[gi * p.ldy + gj] = lines::act_y(h, p.act);
    }
  } else if (MODE == TC_GW) {
    if (gj >= K) return;
    float* out = p.out + (p.split > 1 ? (int64_t)blockIdx.y * p.N * p.ldo : 0);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int gi = at.row(0, e);
      if (gi < p.N) out[(int64_t)gi * p.ldo + gj] = acc[e];
    }
  } else {
    if (gj >= p.C) return;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int64_t sl = at.row(0, e);
      if (sl >= p.total_in) continue;
      const int4 inf = p.info[sl];
      if (inf.x >= 0) p.out[(int64_t)inf.w * p.ldo + gj] = acc[e];
    }
  }
}

template <int MODE>
hipError_t launch_tc_gemm(const TcGemmArgs& a, bool vec, int split, hipStream_t s) {
  const dim3 grid((unsigned)((int64_t)a.nMt * a.nNt), (unsigned)split);
  if (vec) hipLaunchKernelGGL((tc_gemm_kernel<MODE, true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((tc_gemm_kernel<MODE, false>), grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

// gw [N, ldw] (K columns) = the sum of the S planes [N, K] in ascending order, one float32 rounding per addition
__global__ __launch_bounds__(256) void tc_gwsum_kernel(const float* __restrict__ planes, int S, int N, int K, float* __restrict__ gw,
                                                       int64_t ldw) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)N * K) return;
  float v = planes[i];
  for (int s = 1; s < S; ++s) v = __fadd_rn(v, planes[(int64_t)s * N * K + i]);
  gw[i / K * ldw + i % K] = v;
}

// ---------------------------------------------------------------------------------------------- mask, gz, column sums
struct TcMaskArgs {
  const float* gy; int64_t ldgy;
  const float* z; int64_t ldz;
  const int32_t* rowmap;
  int64_t total_out, rows_per_slice;          // slice blockIdx.y takes the rows [y rows_per_slice, (y + 1) rows_per_slice)
  int N, slices;
  const float *gamma, *beta, *mm, *mv;        // all four or none
  int act;
  float* gz; int64_t ldg;                     // [total_out, ldg]
  double* part;                               // [3][N][slices]
};

constexpr int kTcMaskCols = 32;               // columns per workgroup of tc_mask_kernel, 8 per wave

// the twin of seg_mask_kernel (csrc/seg_grad.hip); csrc/layer_lines.h says what they share and why the two bodies stay apart
__global__ __launch_bounds__(256) void tc_mask_kernel(TcMaskArgs p) {
  constexpr int CW = kTcMaskCols / 4;
  __shared__ float ta[64][kTcMaskCols + 1], tz[64][kTcMaskCols + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j0 = (int)blockIdx.x * kTcMaskCols;
  const bool bn = p.gamma != nullptr;
  const int64_t row0 = (int64_t)blockIdx.y * p.rows_per_slice;
  const int64_t row1 = row0 + p.rows_per_slice < p.total_out ? row0 + p.rows_per_slice : p.total_out;
  // phase 1 reads along the rows: a half wave takes 32 columns of one row
  const int c1 = lane & 31, rsub = 2 * wave + (lane >> 5);
  const int jc = j0 + c1;
  const bool jok = jc < p.N;
  float s1 = 1.f, mm1 = 0.f, beta1 = 0.f;
  if (bn && jok) {
    s1 = __fmul_rn(p.gamma[jc], lines::bn_r(p.mv[jc]));
    mm1 = p.mm[jc];
    beta1 = p.beta[jc];
  }
  // phase 2 sums along the columns: wave w owns the columns j0 + 8 w + c, lane = row of the 64-row chunk
  float r2[CW], mm2[CW], s2[CW];
  double sa[CW], sg[CW], sz[CW];
#pragma unroll
  for (int c = 0; c < CW; ++c) {
    const int j = j0 + CW * wave + c;
    s2[c] = 1.f; r2[c] = 0.f; mm2[c] = 0.f;
    sa[c] = sg[c] = sz[c] = 0.0;
    if (j < p.N && bn) {
      r2[c] = lines::bn_r(p.mv[j]);
      s2[c] = __fmul_rn(p.gamma[j], r2[c]);
      mm2[c] = p.mm[j];
    }
  }
  for (int64_t i0 = row0; i0 < row1; i0 += 64) {
    for (int rl = rsub; rl < 64; rl += 8) {
      const int64_t i = i0 + rl;
      float a = 0.f, z = 0.f;
      if (i < row1 && jok && p.rowmap[i] >= 0) {
        z = p.z[i * p.ldz + jc];
        const float h = bn ? lines::bn_h(z, s1, mm1, beta1) : z;
        const float g = p.gy[i * p.ldgy + jc];
        a = lines::act_grad(g, h, p.act);
        p.gz[i * p.ldg + jc] = bn ? __fmul_rn(a, s1) : a;
      }
      ta[rl][c1] = a;
      tz[rl][c1] = z;
    }
    __syncthreads();
    if (i0 + lane < row1) {
#pragma unroll
      for (int c = 0; c < CW; ++c) {
        const int cl = CW * wave + c;
        if (j0 + cl < p.N) {
          const float a = ta[lane][cl];
          const float g = bn ? __fmul_rn(a, s2[c]) : a;          // the bits phase 1 wrote to gz
          sa[c] += (double)a;
          sg[c] += (double)a * ((double)r2[c] * ((double)tz[lane][cl] - (double)mm2[c]));
          sz[c] += (double)g;
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int c = 0; c < CW; ++c) {
    const int j = j0 + CW * wave + c;
    if (j >= p.N) continue;                                       // uniform over the wave
    const double a = wave_sum_f64(sa[c]), g = wave_sum_f64(sg[c]), z = wave_sum_f64(sz[c]);
    if (lane == 0) {
      p.part[((int64_t)0 * p.N + j) * p.slices + blockIdx.y] = a;
      p.part[((int64_t)1 * p.N + j) * p.slices + blockIdx.y] = g;
      p.part[((int64_t)2 * p.N + j) * p.slices + blockIdx.y] = z;
    }
  }
}

__global__ __launch_bounds__(256) void tc_colsum_kernel(const double* __restrict__ part, int N, int slices, int bn, float* __restrict__ gbeta,
                                                        float* __restrict__ ggamma, float* __restrict__ gbias) {
  const int j = (int)(blockIdx.x * 256 + threadIdx.x);
  if (j >= N) return;
  double v[3];
  for (int q = 0; q < 3; ++q) {
    double s = 0.0;
    for (int i = 0; i < slices; ++i) s += part[((int64_t)q * N + j) * slices + i];
    v[q] = s;
  }
  if (bn) {
    gbeta[j] = (float)v[0];
    ggamma[j] = (float)v[1];
  }
  gbias[j] = (float)v[2];
}

// the row slices of the column sums and the row ranges of gw: functions of the shapes and total_out alone
void tc_slices(int64_t total_out, int64_t* rows_per_slice, int* slices) {
  int64_t rows = up((total_out + kTcMaxSlices - 1) / kTcMaxSlices, 64);
  if (rows < 1024) rows = 1024;
  *rows_per_slice = rows;
  *slices = (int)((total_out + rows - 1) / rows);
}

void tc_split(int64_t total_out, int K, int N, int64_t* rows_per_split, int* split) {
  const int64_t tiles = (int64_t)((N + 63) / 64) * ((K + 63) / 64);
  int64_t want = 512 / tiles;                                     // up to two workgroups per compute unit
  if (want > kTcMaxSplit) want = kTcMaxSplit;
  const int64_t most = (total_out + 255) / 256;                   // at least 256 rows per range
  if (want > most) want = most;
  if (want < 1) want = 1;
  const int64_t rows = up((total_out + want - 1) / want, kTcBK);
  *rows_per_split = rows;
  *split = (int)((total_out + rows - 1) / rows);
}

struct TcLayout {
  int64_t ldg;
  int64_t out_off, rowmap, info, part, gz, planes, total;        // byte offsets
};

TcLayout tc_layout(int64_t batch, int64_t total_in, int64_t total_out, int W, int C, int N) {
  TcLayout L;
  int64_t rows, rsplit;
  int slices, split;
  tc_slices(total_out, &rows, &slices);
  tc_split(total_out, W * C, N, &rsplit, &split);
  L.ldg = up(N, 4);
  int64_t o = 0;
  L.out_off = o; o += up(4 * (batch + 1), 256);
  L.rowmap = o;  o += up(4 * total_out, 256);
  L.info = o;    o += up(16 * total_in, 256);
  L.part = o;    o += up((int64_t)8 * 3 * N * slices, 256);
  L.gz = o;      o += up(4 * total_out * L.ldg, 256);
  L.planes = o;  o += split > 1 ? up((int64_t)4 * split * N * W * C, 256) : 0;
  L.total = o;
  return L;
}

hipError_t tc_maps(const int32_t* offsets, int64_t batch, int64_t total_in, int64_t total_out, int W, int32_t* out_off,
                   int32_t* rowmap, int4* info, hipStream_t s) {
  hipLaunchKernelGGL(tc_scan_kernel, dim3(1), dim3(256), 0, s, offsets, batch, W, out_off);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int64_t most = info && total_in > total_out ? total_in : total_out;
  hipLaunchKernelGGL(tc_map_kernel, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, s, offsets, (const int32_t*)out_off, batch,
                     total_out, info ? total_in : 0, rowmap, info);
  return hipGetLastError();
}

}  // namespace

int64_t tconv_workspace_bytes(int64_t batch, int64_t total_in, int64_t total_out, int W, int C, int N) {
  if (batch <= 0 || total_out <= 0 || total_in <= 0 || W <= 0 || C <= 0 || N <= 0) return 0;
  return tc_layout(batch, total_in, total_out, W, C, N).total;
}

int64_t tconv_forward_workspace_bytes(int64_t batch, int64_t total_out) {
  if (batch <= 0 || total_out <= 0) return 0;
  return up(4 * (batch + 1), 256) + up(4 * total_out, 256);      // out_off and rowmap, the head of tc_layout
}

hipError_t launch_tconv_forward(const float* x, int64_t ldx, int C, int W, const int32_t* offsets, int64_t batch, int64_t total_in,
                                int64_t total_out, const float* w, int64_t ldw, int N, const float* bias, const float* gamma,
                                const float* beta, const float* mm, const float* mv, int act, float* z, int64_t ldz, float* y,
                                int64_t ldy, void* ws, hipStream_t s) {
  const TcLayout L = tc_layout(batch, total_in, total_out, W, C, N);
  char* wsb = static_cast<char*>(ws);
  int32_t* out_off = reinterpret_cast<int32_t*>(wsb + L.out_off);
  int32_t* rowmap = reinterpret_cast<int32_t*>(wsb + L.rowmap);
  hipError_t e = tc_maps(offsets, batch, total_in, total_out, W, out_off, rowmap, nullptr, s);
  if (e != hipSuccess) return e;
  TcGemmArgs a = {};
  a.x = x; a.ldx = ldx; a.C = C; a.W = W; a.w = w; a.ldw = ldw; a.N = N;
  a.rowmap = rowmap; a.total_out = total_out;
  a.nMt = (int)((total_out + 63) / 64); a.nNt = (N + 63) / 64;
  a.bias = bias; a.gamma = gamma; a.beta = beta; a.mm = mm; a.mv = mv; a.act = act;
  a.z = z; a.ldz = ldz; a.y = y; a.ldy = ldy;
  const bool vec = aligned16(x) && ldx % 4 == 0 && C % 4 == 0 && aligned16(w) && ldw % 4 == 0;
  return launch_tc_gemm<TC_FWD>(a, vec, 1, s);
}

hipError_t launch_tconv_backward(const float* gy, int64_t ldgy, const float* x, int64_t ldx, int C, int W, const int32_t* offsets,
                                 int64_t batch, int64_t total_in, int64_t total_out, const float* z, int64_t ldz, const float* w,
                                 int64_t ldw, int N, const float* gamma, const float* beta, const float* mm, const float* mv, int act,
                                 float* gx, int64_t ldgx, float* gw, float* gbias, float* ggamma, float* gbeta, void* ws,
                                 hipStream_t s) {
  const int K = W * C;
  const TcLayout L = tc_layout(batch, total_in, total_out, W, C, N);
  char* wsb = static_cast<char*>(ws);
  int32_t* out_off = reinterpret_cast<int32_t*>(wsb + L.out_off);
  int32_t* rowmap = reinterpret_cast<int32_t*>(wsb + L.rowmap);
  int4* info = reinterpret_cast<int4*>(wsb + L.info);
  double* part = reinterpret_cast<double*>(wsb + L.part);
  float* gz = reinterpret_cast<float*>(wsb + L.gz);
  float* planes = reinterpret_cast<float*>(wsb + L.planes);
  hipError_t e = tc_maps(offsets, batch, total_in, total_out, W, out_off, rowmap, gx ? info : nullptr, s);
  if (e != hipSuccess) return e;

  TcMaskArgs m = {};
  m.gy = gy; m.ldgy = ldgy; m.z = z; m.ldz = ldz; m.rowmap = rowmap; m.total_out = total_out; m.N = N;
  tc_slices(total_out, &m.rows_per_slice, &m.slices);
  m.gamma = gamma; m.beta = beta; m.mm = mm; m.mv = mv; m.act = act;
  m.gz = gz; m.ldg = L.ldg; m.part = part;
  hipLaunchKernelGGL(tc_mask_kernel, dim3((unsigned)((N + kTcMaskCols - 1) / kTcMaskCols), (unsigned)m.slices), dim3(256), 0, s, m);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(tc_colsum_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, (const double*)part, N, m.slices,
                     gamma ? 1 : 0, gbeta, ggamma, gbias);
  if ((e = hipGetLastError()) != hipSuccess) return e;

  const bool vec_x = aligned16(x) && ldx % 4 == 0 && C % 4 == 0;
  TcGemmArgs a = {};
  a.x = x; a.ldx = ldx; a.C = C; a.W = W; a.w = w; a.ldw = ldw; a.N = N;
  a.rowmap = rowmap; a.total_out = total_out; a.info = info; a.total_in = total_in;
  a.gz = gz; a.ldg = L.ldg;

  TcGemmArgs c = a;
  tc_split(total_out, K, N, &c.rows_per_split, &c.split);
  c.nMt = (N + 63) / 64; c.nNt = (K + 63) / 64;
  c.out = c.split > 1 ? planes : gw;
  c.ldo = c.split > 1 ? K : ldw;
  if ((e = launch_tc_gemm<TC_GW>(c, vec_x, c.split, s)) != hipSuccess) return e;
  if (c.split > 1) {
    hipLaunchKernelGGL(tc_gwsum_kernel, dim3((unsigned)(((int64_t)N * K + 255) / 256)), dim3(256), 0, s, (const float*)planes, c.split,
                       N, K, gw, ldw);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (gx) {
    TcGemmArgs b = a;
    b.nMt = (int)((total_in + 63) / 64); b.nNt = (C + 63) / 64;
    b.out = gx; b.ldo = ldgx;
    const bool vec_w = aligned16(w) && ldw % 4 == 0 && C % 4 == 0;
    if ((e = launch_tc_gemm<TC_GX>(b, vec_w, 1, s)) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace xv
