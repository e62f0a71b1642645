// Forward and backward of one 2-D ("grid") convolution of the ResNet on packed utterances: tf.layers.conv2d(.., (kh, kw), strides
// (st, sf), padding='same') of model/resnet.py + batch norm (inference mode) + activation, with the CURRENT weights; and the
// residual join of a block, y = act(p + q), with its gradient.  It is the grid twin of csrc/tconv_grad.hip: the rule is stated in
// include/xvec_hip.h (xv_gconv_forward, xv_gconv_backward, xv_add_act_forward, xv_add_act_backward) and restated in float64
// numpy in tests/helpers/ref_gconv.py; torch.autograd of F.pad + F.conv2d + eval-mode batch_norm + relu / leaky_relu(0.2) gives
// the same numbers (tests/test_gconv_host.py).
//
// Rows are (utterance, frame, bin): element (l, f) of utterance b is row (offsets[b] + l) F_in + f of x; an utterance of L frames
// gives L_out = ceil(L / st) frames of F_out = ceil(F_in / sf) bins, packed from frame 0.  Nothing is unfolded and nothing is
// scattered.  Row o of the im2col matrix X [rows_out, K = kh kw C] is a VIEW of x: element k = (dl kw + df) C + c is channel c of
// the input bin (lo st - pad_t + dl, fo sf - pad_f + df), a zero operand where that bin lies outside the utterance's own frames or
// outside [0, F_in) (TensorFlow's 'same': pad = max((out - 1) s + k - in, 0) / 2 zeros in front, per utterance along time).  All
// three products are exact-fp32 GEMMs on v_mfma_f32_32x32x2_f32 over such views: the loop of csrc/tconv_grad.hip (64 x 64 tiles,
// a reduction step of 32, zero-filled edges, register-staged double buffering, NtPos of csrc/nt_gemm.h) with the 2-D gather in
// the tile loaders.
//  * gc_scan_kernel, gc_map_kernel: out_off[b] = sum_{a < b} ceil(L_a / st) on the device; then for every output row (first frame
//    of its utterance, L, lo st - pad_t, fo sf - pad_f), L = 0 beyond the last output row, and for every owned input row (its
//    frame in its utterance, out_off, L_out, pad_t), frame -1 beyond the last owned row.  The row maps are precomputed in the
//    workspace: a loader reads one int4 per staging row and tile, not per element.
//  * gc_gemm_kernel<GC_FWD>: z = X . w^T (+ b), then h and y by the lines of csrc/layer_lines.h.  The chain of z runs over k
//    ascending from 0, a function of kh kw C alone; the bias, if there is one, comes last.  conv0_1 (C = 1, K = 9) takes this
//    kernel as well, with one reduction step padded by exact zeros: no direct kernel (0.3 % of a step's products).
//  * gc_mask_kernel, gc_colsum_kernel: a = gy act'(h), gz = a s_j written once as gz [rows_out, round4(N)], and the three column
//    sums in double, in the slice order of xv_tconv_backward (gc_slices = tc_slices).
//  * gc_gemm_kernel<GC_GW>: gw = gz^T . X, the chain over the output rows ascending, cut into S contiguous ranges (gc_split, below)
//    that sum into their own planes from zero; gc_gwsum_kernel adds the planes in ascending order, one rounding each.
//  * gc_gemm_kernel<GC_GX>: gx [input rows, C] = G . w', row i of G the gather of gz at the output bins that read input bin i: tap
//    (dl, df) contributes where l + pad_t - dl is a multiple of st with a quotient in [0, L_out), and likewise f + pad_f - df along
//    frequency; w'[tap round4(N) + j][c] = w[j][tap C + c] read in place.  One writer per element: a gather, not a col2im scatter.
//    The chain runs over the taps ascending, then j ascending; an input bin no output reads (odd positions under a strided 1 x 1)
//    is a chain of exact zeros.  Under a stride most taps of a row are zero operands: they are multiplied, not skipped.
// The row split of gw.  tc_split's cap of 32 ranges was sized for 18 k rows; the first stage of the ResNet has 768 000 output rows
// and nine tiles.  S' = max(1, min(ceil(1024 / tiles), 256, ceil(rows_out / 1024))), tiles = ceil(N / 64) ceil(K / 64): about four
// workgroups per compute unit where the tiles alone give fewer, never a range below 1024 rows, at most 256 planes; the ranges
// hold ceil32(ceil(rows_out / S')) rows.  A function of N, K and total_out alone.
// Every element of every output is a function of the inputs alone: one writer per element, a fixed order, no floating-point
// atomics, no value read from memory this call did not write.  z, y and gx of an utterance use its own rows and the parameters
// only.  Nothing of the workspace depends on ws_bytes.
//
// Error bound (u = 2^-24; checked per element in tests/test_gpu_gconv.py, restated in ref_gconv.bounds).  |.| of the float64
// oracle's values; n = the output rows, X the gathered view, K = kh kw C, T = kh kw; the forms of csrc/tconv_grad.hip:
//   z_ij:      Bz = (K + 2) u (sum_k |X_ik w_jk| + |b_j|)                     (fmaf chain of length K, then the bias)
//   h, y, a, gz, gbeta, ggamma, gbias: the bounds of csrc/layer_lines.h with this Bz
//   gw_jk:     sum_i Bg |X_ik| + (n + 64) u sum_i |gz_ij X_ik|               (S chains of at most n / S + 32 steps, then S - 1
//              additions; S <= n / 1024 + 1, so n / S + 31 + S <= n + 64)
//   gx_ic:     sum_{tap, j} Bg |w_j,tap C + c| + (T (N + 3) + 2) u sum_{tap, j} |gz_{o(i, tap), j} w_j,tap C + c|
// The residual join is one float32 addition and act_y / act_grad: y and g carry u |p + q| through the activation and the
// roundings of layer_lines.h; its outputs are the bits of numpy float32 written the same way.
#include "layer_lines.h"
#include "nt_gemm.h"

namespace xv {

using ntg::gf32x16;
using ntg::gf32x4;
using ntg::up;

namespace {

constexpr int kGcTile = 64;
constexpr int kGcBK = 32;
constexpr int kGcLdRow = kGcBK + 4;           // operand tile [64 rows][32 k + 4]
constexpr int kGcLdRed = kGcTile + 8;         // operand tile [32 k][64 rows + 8]
constexpr int kGcTileFloats = kGcTile * kGcLdRow;
static_assert(kGcBK * kGcLdRed == kGcTileFloats, "both tile kinds take the same LDS");
constexpr int kGcMaxSplit = 256;
constexpr int kGcMaxSlices = 64;

enum { GC_FWD = 0, GC_GW = 1, GC_GX = 2 };

// the shape of one convolution: bins in and out, the window, the strides (1 or 2, so st - 1 and sf - 1 are shifts and masks),
// the zeros in front along frequency
struct GcGeom {
  int F_in, F_out, kh, kw, st, sf, pf, C;
};

__host__ __device__ inline int gc_out(int n, int s) { return (n + s - 1) / s; }
__host__ __device__ inline int gc_pad(int n, int k, int s) {
  const int t = (gc_out(n, s) - 1) * s + k - n;
  return t > 0 ? t / 2 : 0;
}

// ---------------------------------------------------------------------------------------------- offsets and row maps
// out_off [batch + 1] in frames: one workgroup walks the utterances in chunks of 256 with a running carry
__global__ __launch_bounds__(256) void gc_scan_kernel(const int32_t* __restrict__ in_off, int64_t batch, int st, int32_t* __restrict__ out_off) {
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
      v = in_off[b + 1] - in_off[b];
      v = v > 0 ? gc_out(v, st) : 0;
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

// the utterance that owns frame v of an ascending offsets array: the last b with off[b] <= v (off[0] <= v < off[batch])
__device__ __forceinline__ int64_t gc_owner(const int32_t* off, int64_t batch, int64_t v) {
  int64_t lo = 0, hi = batch;                 // off[lo] <= v < off[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid] <= v) lo = mid; else hi = mid;
  }
  return lo;
}

// omap [rows_out]: (first input frame of the utterance, its L, lo st - pad_t, fo sf - pad_f); L = 0 beyond the last output row.
// imap [rows_in]: for input row in_off[0] F_in + i: (its frame in its utterance, out_off of the utterance, L_out, pad_t);
// frame -1 beyond the last owned row.
__global__ __launch_bounds__(256) void gc_map_kernel(const int32_t* __restrict__ in_off, const int32_t* __restrict__ out_off,
                                                     int64_t batch, int64_t rows_out, int64_t rows_in, GcGeom g, int4* __restrict__ omap,
                                                     int4* __restrict__ imap) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < rows_out) {
    int4 v = make_int4(0, 0, 0, 0);
    const int64_t fr = i / g.F_out;
    if (fr < out_off[batch]) {
      const int64_t b = gc_owner(out_off, batch, fr);
      const int L = in_off[b + 1] - in_off[b];
      const int lo = (int)(fr - out_off[b]), fo = (int)(i - fr * g.F_out);
      v = make_int4(in_off[b], L, lo * g.st - gc_pad(L, g.kh, g.st), fo * g.sf - g.pf);
    }
    omap[i] = v;
  }
  if (imap && i < rows_in) {
    int4 v = make_int4(-1, 0, 0, 0);
    const int64_t s = (int64_t)in_off[0] + i / g.F_in;
    if (s < in_off[batch]) {
      const int64_t b = gc_owner(in_off, batch, s);
      const int L = in_off[b + 1] - in_off[b];
      v = make_int4((int)(s - in_off[b]), out_off[b], out_off[b + 1] - out_off[b], gc_pad(L, g.kh, g.st));
    }
    imap[i] = v;
  }
}

// ---------------------------------------------------------------------------------------------- the three products
struct GcGemmArgs {
  const float* x; int64_t ldx; GcGeom g;      // the packed input, K = kh kw C
  const float* w; int64_t ldw; int N;         // [N, ldw], K columns
  const int32_t* in_off;                      // offsets[0] places the rows of gx
  const int4* omap; int64_t rows_out;
  const int4* imap; int64_t rows_in;
  const float* gz; int64_t ldg;               // [rows_out, ldg]
  int nMt, nNt;
  // GC_FWD
  const float *bias, *gamma, *beta, *mm, *mv;
  int act;
  float* z; int64_t ldz; float* y; int64_t ldy;
  // GC_GW: split s takes the output rows [s rows_per_split, (s + 1) rows_per_split); out = gw, or the planes when split > 1
  int split; int64_t rows_per_split;
  // GC_GW, GC_GX
  float* out; int64_t ldo;
};

// four consecutive elements k .. k + 3 of the gathered row of the output bin with map m (k < K, a multiple of 4)
template <bool VEC>
__device__ __forceinline__ gf32x4 gc_load_x(const float* __restrict__ x, int64_t ldx, const GcGeom& g, int K, const int4& m, int k) {
  gf32x4 v = {0.f, 0.f, 0.f, 0.f};
  int tap = k / g.C, c = k - tap * g.C;
  if (VEC) {                                  // C % 4 == 0: one tap, 16-byte aligned
    const int dl = tap / g.kw, df = tap - dl * g.kw;
    const int l = m.z + dl, f = m.w + df;
    if (l >= 0 && l < m.y && f >= 0 && f < g.F_in)
      v = *reinterpret_cast<const gf32x4*>(x + (((int64_t)m.x + l) * g.F_in + f) * ldx + c);
    return v;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (k + e < K) {
      const int dl = tap / g.kw, df = tap - dl * g.kw;
      const int l = m.z + dl, f = m.w + df;
      if (l >= 0 && l < m.y && f >= 0 && f < g.F_in) v[e] = x[(((int64_t)m.x + l) * g.F_in + f) * ldx + c];
    }
    if (++c == g.C) { c = 0; ++tap; }
  }
  return v;
}

// the row of gz that tap (dl, df) of input bin (inf.x, f) reads, -1 where the tap contributes nothing
__device__ __forceinline__ int64_t gc_gz_row(const GcGeom& g, const int4& inf, int f, int tap) {
  const int dl = tap / g.kw, df = tap - dl * g.kw;
  const int tl = inf.x + inf.w - dl, tf = f + g.pf - df;
  if (tl < 0 || tf < 0 || (tl & (g.st - 1)) || (tf & (g.sf - 1))) return -1;
  const int lo = tl >> (g.st - 1), fo = tf >> (g.sf - 1);
  if (lo >= inf.z || fo >= g.F_out) return -1;
  return ((int64_t)inf.y + lo) * g.F_out + fo;
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(256, 2) void gc_gemm_kernel(GcGemmArgs p) {
  // A and B, two buffers each.  Tile kinds: GC_FWD A rows, B rows; GC_GW A red, B red; GC_GX A rows, B red.
  __shared__ __attribute__((aligned(16))) float smem[4 * kGcTileFloats];
  constexpr bool A_RED = MODE == GC_GW, B_RED = MODE != GC_FWD;
  float* As = smem;
  float* Bs = smem + 2 * kGcTileFloats;
  const int mt = (int)(blockIdx.x % (unsigned)p.nMt), nt = (int)(blockIdx.x / (unsigned)p.nMt);
  const ntg::NtPos<64, 64> at(mt, nt);
  const int tid = threadIdx.x;
  const GcGeom g = p.g;
  const int T = g.kh * g.kw, K = T * g.C;

  // staging coordinates: a rows tile takes (row lr + 32 i, k 4 c4), a red tile (k kr + 16 i, row 4 c16)
  const int c4 = tid & 7, lr = tid >> 3;
  const int c16 = tid & 15, kr = tid >> 4;

  // the reduction: its range and what each thread keeps of its two staging rows
  int64_t red0 = 0, red1 = 0;
  int4 amap[2];                               // GC_FWD: the map of the output row; GC_GX: of the input row
  int af[2] = {0, 0};                         // GC_GX: the bin of the input row
  amap[0] = amap[1] = make_int4(MODE == GC_GX ? -1 : 0, 0, 0, 0);
  if (MODE == GC_FWD) {
    red1 = K;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t r = (int64_t)at.m0 + lr + 32 * i;
      if (r < p.rows_out) amap[i] = p.omap[r];
    }
  } else if (MODE == GC_GW) {
    red0 = (int64_t)blockIdx.y * p.rows_per_split;
    red1 = red0 + p.rows_per_split < p.rows_out ? red0 + p.rows_per_split : p.rows_out;
  } else {
    red1 = (int64_t)T * p.ldg;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t sl = (int64_t)at.m0 + lr + 32 * i;
      if (sl < p.rows_in) {
        amap[i] = p.imap[sl];
        af[i] = (int)(sl % g.F_in);
      }
    }
  }
  const int nk = (int)((red1 - red0 + kGcBK - 1) / kGcBK);

  gf32x4 ra[2], rb[2];
  auto load_tiles = [&](int kt) {
    const int64_t k0 = red0 + (int64_t)kt * kGcBK;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      gf32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
      if (MODE == GC_FWD) {
        const int k = (int)k0 + 4 * c4;
        if (amap[i].y > 0 && k < K) a = gc_load_x<VEC>(p.x, p.ldx, g, K, amap[i], k);
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
      } else if (MODE == GC_GW) {
        const int64_t r = k0 + kr + 16 * i;
        int4 m = make_int4(0, 0, 0, 0);
        if (r < red1) m = p.omap[r];
        const int j = at.m0 + 4 * c16, k = at.n0 + 4 * c16;
        if (m.y > 0) {
          if (j < p.N) a = *reinterpret_cast<const gf32x4*>(p.gz + r * p.ldg + j);      // columns N .. ldg feed rows never stored
          if (k < K) b = gc_load_x<VEC>(p.x, p.ldx, g, K, m, k);
        }
      } else {
        {
          const int64_t kk = k0 + 4 * c4;                        // tap ldg + j, j a multiple of 4
          const int tap = (int)(kk / p.ldg), j = (int)(kk - (int64_t)tap * p.ldg);
          if (kk < red1 && amap[i].x >= 0 && j < p.N) {
            const int64_t row = gc_gz_row(g, amap[i], af[i], tap);
            if (row >= 0) {
              a = *reinterpret_cast<const gf32x4*>(p.gz + row * p.ldg + j);
#pragma unroll
              for (int e = 1; e < 4; ++e)
                if (j + e >= p.N) a[e] = 0.f;                     // the padding columns of gz hold nothing
            }
          }
        }
        const int64_t kk = k0 + kr + 16 * i;
        const int tap = (int)(kk / p.ldg), j = (int)(kk - (int64_t)tap * p.ldg);
        const int c = at.n0 + 4 * c16;
        if (kk < red1 && j < p.N && c < g.C) {
          const float* src = p.w + (int64_t)j * p.ldw + (int64_t)tap * g.C + c;
          if (VEC) {
            b = *reinterpret_cast<const gf32x4*>(src);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (c + e < g.C) b[e] = src[e];
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
      float* da = As + buf * kGcTileFloats + (A_RED ? (kr + 16 * i) * kGcLdRed + 4 * c16 : (lr + 32 * i) * kGcLdRow + 4 * c4);
      float* db = Bs + buf * kGcTileFloats + (B_RED ? (kr + 16 * i) * kGcLdRed + 4 * c16 : (lr + 32 * i) * kGcLdRow + 4 * c4);
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
    const float* ap = As + cur * kGcTileFloats;
    const float* bp = Bs + cur * kGcTileFloats;
#pragma unroll
    for (int q = 0; q < kGcBK / 8; ++q) {
      // lane (r, h) feeds k = 8 q + 4 h + j of both operands: the order of the chain is a function of k alone
      gf32x4 a, b;
      if (A_RED) {
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = ap[(8 * q + 4 * at.h + j) * kGcLdRed + arow_l];
      } else {
        a = *reinterpret_cast<const gf32x4*>(ap + arow_l * kGcLdRow + 8 * q + 4 * at.h);
      }
      if (B_RED) {
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = bp[(8 * q + 4 * at.h + j) * kGcLdRed + brow_l];
      } else {
        b = *reinterpret_cast<const gf32x4*>(bp + brow_l * kGcLdRow + 8 * q + 4 * at.h);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
    }
    if (kt + 1 < nk) store_tiles(cur ^ 1);
    __syncthreads();
  }

  const int gj = at.col(0);
  if (MODE == GC_FWD) {
    if (gj >= p.N) return;
    float s = 0.f, mm = 0.f, beta = 0.f;
    if (p.gamma) {
      s = __fmul_rn(p.gamma[gj], lines::bn_r(p.mv[gj]));
      mm = p.mm[gj];
      beta = p.beta[gj];
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int64_t gi = at.row(0, e);
      if (gi >= p.rows_out || p.omap[gi].y <= 0) continue;
      const float z = p.bias ? __fadd_rn(acc[e], p.bias[gj]) : acc[e];
      const float h = p.gamma ? lines::bn_h(z, s, mm, beta) : z;
      p.z[gi * p.ldz + gj] = z;
      p.y[gi * p.ldy + gj] = lines::act_y(h, p.act);
    }
  } else if (MODE == GC_GW) {
    if (gj >= K) return;
    float* out = p.out + (p.split > 1 ? (int64_t)blockIdx.y * p.N * p.ldo : 0);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int gi = at.row(0, e);
      if (gi < p.N) out[(int64_t)gi * p.ldo + gj] = acc[e];
    }
  } else {
    if (gj >= g.C) return;
    const int64_t row0 = (int64_t)p.in_off[0] * g.F_in;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int64_t sl = at.row(0, e);
      if (sl >= p.rows_in) continue;
      if (p.imap[sl].x >= 0) p.out[(row0 + sl) * p.ldo + gj] = acc[e];
    }
  }
}

template <int MODE>
hipError_t launch_gc_gemm(const GcGemmArgs& a, bool vec, int split, hipStream_t s) {
  const dim3 grid((unsigned)((int64_t)a.nMt * a.nNt), (unsigned)split);
  if (vec) hipLaunchKernelGGL((gc_gemm_kernel<MODE, true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((gc_gemm_kernel<MODE, false>), grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

// gw [N, ldw] (K columns) = the sum of the S planes [N, K] in ascending order, one float32 rounding per addition
__global__ __launch_bounds__(256) void gc_gwsum_kernel(const float* __restrict__ planes, int S, int N, int K, float* __restrict__ gw,
                                                       int64_t ldw) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)N * K) return;
  float v = planes[i];
  for (int s = 1; s < S; ++s) v = __fadd_rn(v, planes[(int64_t)s * N * K + i]);
  gw[i / K * ldw + i % K] = v;
}

// ---------------------------------------------------------------------------------------------- mask, gz, column sums
struct GcMaskArgs {
  const float* gy; int64_t ldgy;
  const float* z; int64_t ldz;
  const int4* omap;
  int64_t rows_out, rows_per_slice;           // slice blockIdx.y takes the rows [y rows_per_slice, (y + 1) rows_per_slice)
  int N, slices;
  const float *gamma, *beta, *mm, *mv;        // all four or none
  int act;
  float* gz; int64_t ldg;                     // [rows_out, ldg]
  double* part;                               // [3][N][slices]
};

constexpr int kGcMaskCols = 32;               // columns per workgroup of gc_mask_kernel, 8 per wave

// the twin of tc_mask_kernel (csrc/tconv_grad.hip); csrc/layer_lines.h says what they share and why the bodies stay apart
__global__ __launch_bounds__(256) void gc_mask_kernel(GcMaskArgs p) {
  constexpr int CW = kGcMaskCols / 4;
  __shared__ float ta[64][kGcMaskCols + 1], tz[64][kGcMaskCols + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j0 = (int)blockIdx.x * kGcMaskCols;
  const bool bn = p.gamma != nullptr;
  const int64_t row0 = (int64_t)blockIdx.y * p.rows_per_slice;
  const int64_t row1 = row0 + p.rows_per_slice < p.rows_out ? row0 + p.rows_per_slice : p.rows_out;
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
      if (i < row1 && jok && p.omap[i].y > 0) {
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

// gbias may be null: the ResNet's grid convolutions have no bias
__global__ __launch_bounds__(256) void gc_colsum_kernel(const double* __restrict__ part, int N, int slices, int bn, float* __restrict__ gbeta,
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
  if (gbias) gbias[j] = (float)v[2];
}

// the row slices of the column sums (those of tc_slices) and the row ranges of gw: functions of the shapes and rows_out alone
void gc_slices(int64_t rows_out, int64_t* rows_per_slice, int* slices) {
  int64_t rows = up((rows_out + kGcMaxSlices - 1) / kGcMaxSlices, 64);
  if (rows < 1024) rows = 1024;
  *rows_per_slice = rows;
  *slices = (int)((rows_out + rows - 1) / rows);
}

void gc_split(int64_t rows_out, int K, int N, int64_t* rows_per_split, int* split) {
  const int64_t tiles = (int64_t)((N + 63) / 64) * ((K + 63) / 64);
  int64_t want = (1024 + tiles - 1) / tiles;                      // about four workgroups per compute unit
  if (want > kGcMaxSplit) want = kGcMaxSplit;
  const int64_t most = (rows_out + 1023) / 1024;                  // no range below 1024 rows
  if (want > most) want = most;
  if (want < 1) want = 1;
  const int64_t rows = up((rows_out + want - 1) / want, kGcBK);
  *rows_per_split = rows;
  *split = (int)((rows_out + rows - 1) / rows);
}

struct GcLayout {
  int64_t ldg;
  int64_t out_off, omap, imap, part, gz, planes, total;          // byte offsets
};

GcLayout gc_layout(int64_t batch, int64_t rows_in, int64_t rows_out, int K, int N) {
  GcLayout L;
  int64_t rows, rsplit;
  int slices, split;
  gc_slices(rows_out, &rows, &slices);
  gc_split(rows_out, K, N, &rsplit, &split);
  L.ldg = up(N, 4);
  int64_t o = 0;
  L.out_off = o; o += up(4 * (batch + 1), 256);
  L.omap = o;    o += up(16 * rows_out, 256);
  L.imap = o;    o += up(16 * rows_in, 256);
  L.part = o;    o += up((int64_t)8 * 3 * N * slices, 256);
  L.gz = o;      o += up(4 * rows_out * L.ldg, 256);
  L.planes = o;  o += split > 1 ? up((int64_t)4 * split * N * K, 256) : 0;
  L.total = o;
  return L;
}

GcGeom gc_geom(int F_in, int kh, int kw, int st, int sf, int C) {
  GcGeom g;
  g.F_in = F_in; g.F_out = gc_out(F_in, sf); g.kh = kh; g.kw = kw; g.st = st; g.sf = sf; g.pf = gc_pad(F_in, kw, sf); g.C = C;
  return g;
}

hipError_t gc_maps(const int32_t* offsets, int64_t batch, int64_t rows_in, int64_t rows_out, const GcGeom& g, int32_t* out_off,
                   int4* omap, int4* imap, hipStream_t s) {
  hipLaunchKernelGGL(gc_scan_kernel, dim3(1), dim3(256), 0, s, offsets, batch, g.st, out_off);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int64_t most = imap && rows_in > rows_out ? rows_in : rows_out;
  hipLaunchKernelGGL(gc_map_kernel, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, s, offsets, (const int32_t*)out_off, batch,
                     rows_out, imap ? rows_in : 0, g, omap, imap);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- the residual join
struct AddActArgs {
  const float* gy; int64_t ldgy;              // null in the forward
  const float* p; int64_t ldp;
  const float* q; int64_t ldq;
  int64_t rows; int N; int act;
  float* out; int64_t ldo;
};

template <bool BWD>
__global__ __launch_bounds__(256) void add_act_kernel(AddActArgs a) {
  const int64_t total = a.rows * a.N, step = (int64_t)gridDim.x * 256;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += step) {
    const int64_t i = e / a.N;
    const int j = (int)(e - i * a.N);
    const float h = __fadd_rn(a.p[i * a.ldp + j], a.q[i * a.ldq + j]);
    a.out[i * a.ldo + j] = BWD ? lines::act_grad(a.gy[i * a.ldgy + j], h, a.act) : lines::act_y(h, a.act);
  }
}

}  // namespace

int64_t gconv_workspace_bytes(int64_t batch, int64_t total_in, int64_t total_out, int F_in, int kh, int kw, int st, int sf, int C,
                              int N) {
  if (batch <= 0 || total_out <= 0 || total_in <= 0 || F_in <= 0 || C <= 0 || N <= 0) return 0;
  return gc_layout(batch, total_in * F_in, total_out * gc_out(F_in, sf), kh * kw * C, N).total;
}

int64_t gconv_forward_workspace_bytes(int64_t batch, int64_t total_out, int F_in, int sf) {
  if (batch <= 0 || total_out <= 0 || F_in <= 0) return 0;
  return up(4 * (batch + 1), 256) + up(16 * total_out * gc_out(F_in, sf), 256);       // out_off and omap, the head of gc_layout
}

hipError_t launch_gconv_forward(const float* x, int64_t ldx, int C, int F_in, int kh, int kw, int st, int sf, const int32_t* offsets,
                                int64_t batch, int64_t total_in, int64_t total_out, const float* w, int64_t ldw, int N,
                                const float* bias, const float* gamma, const float* beta, const float* mm, const float* mv, int act,
                                float* z, int64_t ldz, float* y, int64_t ldy, void* ws, hipStream_t s) {
  const GcGeom g = gc_geom(F_in, kh, kw, st, sf, C);
  const int64_t rows_in = total_in * F_in, rows_out = total_out * g.F_out;
  const GcLayout L = gc_layout(batch, rows_in, rows_out, kh * kw * C, N);
  char* wsb = static_cast<char*>(ws);
  int32_t* out_off = reinterpret_cast<int32_t*>(wsb + L.out_off);
  int4* omap = reinterpret_cast<int4*>(wsb + L.omap);
  hipError_t e = gc_maps(offsets, batch, rows_in, rows_out, g, out_off, omap, nullptr, s);
  if (e != hipSuccess) return e;
  GcGemmArgs a = {};
  a.x = x; a.ldx = ldx; a.g = g; a.w = w; a.ldw = ldw; a.N = N; a.in_off = offsets;
  a.omap = omap; a.rows_out = rows_out;
  a.nMt = (int)((rows_out + 63) / 64); a.nNt = (N + 63) / 64;
  a.bias = bias; a.gamma = gamma; a.beta = beta; a.mm = mm; a.mv = mv; a.act = act;
  a.z = z; a.ldz = ldz; a.y = y; a.ldy = ldy;
  const bool vec = aligned16(x) && ldx % 4 == 0 && C % 4 == 0 && aligned16(w) && ldw % 4 == 0;
  return launch_gc_gemm<GC_FWD>(a, vec, 1, s);
}

hipError_t launch_gconv_backward(const float* gy, int64_t ldgy, const float* x, int64_t ldx, int C, int F_in, int kh, int kw, int st,
                                 int sf, const int32_t* offsets, int64_t batch, int64_t total_in, int64_t total_out, const float* z,
                                 int64_t ldz, const float* w, int64_t ldw, int N, const float* gamma, const float* beta,
                                 const float* mm, const float* mv, int act, float* gx, int64_t ldgx, float* gw, float* gbias,
                                 float* ggamma, float* gbeta, void* ws, hipStream_t s) {
  const GcGeom g = gc_geom(F_in, kh, kw, st, sf, C);
  const int K = kh * kw * C;
  const int64_t rows_in = total_in * F_in, rows_out = total_out * g.F_out;
  const GcLayout L = gc_layout(batch, rows_in, rows_out, K, N);
  char* wsb = static_cast<char*>(ws);
  int32_t* out_off = reinterpret_cast<int32_t*>(wsb + L.out_off);
  int4* omap = reinterpret_cast<int4*>(wsb + L.omap);
  int4* imap = reinterpret_cast<int4*>(wsb + L.imap);
  double* part = reinterpret_cast<double*>(wsb + L.part);
  float* gz = reinterpret_cast<float*>(wsb + L.gz);
  float* planes = reinterpret_cast<float*>(wsb + L.planes);
  hipError_t e = gc_maps(offsets, batch, rows_in, rows_out, g, out_off, omap, gx ? imap : nullptr, s);
  if (e != hipSuccess) return e;

  GcMaskArgs m = {};
  m.gy = gy; m.ldgy = ldgy; m.z = z; m.ldz = ldz; m.omap = omap; m.rows_out = rows_out; m.N = N;
  gc_slices(rows_out, &m.rows_per_slice, &m.slices);
  m.gamma = gamma; m.beta = beta; m.mm = mm; m.mv = mv; m.act = act;
  m.gz = gz; m.ldg = L.ldg; m.part = part;
  hipLaunchKernelGGL(gc_mask_kernel, dim3((unsigned)((N + kGcMaskCols - 1) / kGcMaskCols), (unsigned)m.slices), dim3(256), 0, s, m);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(gc_colsum_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, (const double*)part, N, m.slices,
                     gamma ? 1 : 0, gbeta, ggamma, gbias);
  if ((e = hipGetLastError()) != hipSuccess) return e;

  const bool vec_x = aligned16(x) && ldx % 4 == 0 && C % 4 == 0;
  GcGemmArgs a = {};
  a.x = x; a.ldx = ldx; a.g = g; a.w = w; a.ldw = ldw; a.N = N; a.in_off = offsets;
  a.omap = omap; a.rows_out = rows_out; a.imap = imap; a.rows_in = rows_in;
  a.gz = gz; a.ldg = L.ldg;

  GcGemmArgs c = a;
  gc_split(rows_out, K, N, &c.rows_per_split, &c.split);
  c.nMt = (N + 63) / 64; c.nNt = (K + 63) / 64;
  c.out = c.split > 1 ? planes : gw;
  c.ldo = c.split > 1 ? K : ldw;
  if ((e = launch_gc_gemm<GC_GW>(c, vec_x, c.split, s)) != hipSuccess) return e;
  if (c.split > 1) {
    hipLaunchKernelGGL(gc_gwsum_kernel, dim3((unsigned)(((int64_t)N * K + 255) / 256)), dim3(256), 0, s, (const float*)planes, c.split,
                       N, K, gw, ldw);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (gx) {
    GcGemmArgs b = a;
    b.nMt = (int)((rows_in + 63) / 64); b.nNt = (C + 63) / 64;
    b.out = gx; b.ldo = ldgx;
    const bool vec_w = aligned16(w) && ldw % 4 == 0 && C % 4 == 0;
    if ((e = launch_gc_gemm<GC_GX>(b, vec_w, 1, s)) != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_add_act(const float* gy, int64_t ldgy, const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t rows, int N,
                          int act, float* out, int64_t ldo, hipStream_t s) {
  AddActArgs a = {gy, ldgy, p, ldp, q, ldq, rows, N, act, out, ldo};
  int64_t blocks = (rows * N + 255) / 256;
  if (blocks > (1 << 20)) blocks = 1 << 20;
  if (gy) hipLaunchKernelGGL(add_act_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(add_act_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace xv
