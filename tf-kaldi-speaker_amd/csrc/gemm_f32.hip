// fp32 MFMA GEMM for gfx950 (MI355X): temporal convolution / dense layers of the TDNN as an
// "overlapping-row" GEMM with a fused bias + batch-norm + activation epilogue.
//
//   Y[rowmap[m], n] = act((sum_k A[m,k] * Wt[n,k]) * scale[n] + shift[n]),  A[m,k] = X[m*ldx + k]
//
// replaces tf.layers.conv2d (1,w) / tf.layers.dense + tf.layers.batch_normalization + relu
// (model/tdnn.py:42-130,137-179) with one launch per layer.
//
// Design (CDNA4):
//  * v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate (bitwise an fmaf chain), 64
//    FLOP/clk/SIMD -> 157 TFLOP/s chip peak.  A wave owns a 64x64 output tile = 2x2 MFMA tiles
//    (64 accumulator VGPRs); a 256-thread workgroup owns 128x128; two workgroups per CU.
//  * The K index of an MFMA is only a summation label, so both operands use the same permuted k
//    order: lane (r, h) reads FOUR consecutive k (one ds_read_b128) and feeds them to four
//    successive MFMAs (k = 8q + 4h + j).  One b128 LDS read per operand per 4 MFMAs.
//  * LDS tiles are [row][32 + 4 pad] floats: the 144-byte row stride makes every ds_read_b128
//    lane group hit 16 distinct 16-byte slots (conflict free) and keeps ds_write_b128 aligned.
//  * Register-staged double buffering: the global loads of tile t+1 are issued before the
//    MFMAs of tile t and written to the other LDS buffer after them; one barrier per K tile.
//  * Weights are pre-packed [Npad][Kpad] (k contiguous, zero padded), so the B tile is loaded
//    exactly like the A tile and needs no bounds checks.
//  * XCD-aware block order: consecutive ids on one XCD (id % 8) walk the N tiles of the same M
//    tile, so the A panel is fetched once per XCD L2.
//  * Segment-level layers (M <= 512, dense) have a kernel of their own: gemm_f32_seg_kernel below.
#include <mutex>

#include "xv_epilogue.h"

namespace xv {

constexpr int BM = 128, BN = 128, BK = 32;
constexpr int LDT = BK + 4;               // padded LDS row (floats)
constexpr int TILE_F = BM * LDT;          // floats per operand tile

// FORM: 0 = any shape / alignment (scalar loads), 1 = aligned 1-D rows, 2 = aligned grid form (ResNet taps).  The grid
// addressing is a template case of its own: as a run-time branch in the 1-D loader it cost the TDNN layers 12 %.
template <int FORM>
__global__ __launch_bounds__(256, 2) void gemm_f32_kernel(GemmArgs p, int nMt, int nNt, int kper) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                 // [2][BM][LDT]
  float* Bs = smem + 2 * TILE_F;    // [2][BN][LDT]

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r32 = lane & 31, h = lane >> 5;

  const int ntiles = nMt * nNt;
  const int slice = blockIdx.x / ntiles;                       // split-K slice (0 when off)
  const int tile = xcd_remap(blockIdx.x - slice * ntiles, ntiles);
  const int mt = tile / nNt, nt = tile - mt * nNt;
  const int m0 = mt * BM, n0 = nt * BN;

  // staging map: thread -> (row lr + 32*i, float4 column c4)
  const int c4 = tid & 7, lr = tid >> 3;
  const int kt0 = slice * kper;
  const int nk = min(p.Kpad / BK, kt0 + kper);
  if (p.ksplit > 1) {                                           // raw partial sums of this slice
    p.Y = p.partial + (int64_t)slice * p.M * p.Npad;
    p.ldy = p.Npad;
    p.N = p.Npad;
    p.Ysb = nullptr;
    p.rowmap = nullptr;
    p.raw = 1;
    p.act = ACT_NONE;
    p.R = nullptr;                       // the shortcut is added once, by splitk_reduce_kernel
  }

  f32x4 ra[4], rb[4];
  auto load_tiles = [&](int kt) {
    const int k = kt * BK + c4 * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = lr + 32 * i;
      rb[i] = *reinterpret_cast<const f32x4*>(p.Wt + (int64_t)(n0 + row) * p.Kpad + k);
      if (FORM != 0) {
        if (k >= p.K) {
          ra[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        } else if (FORM == 2) {        // grid form: A[m, tap*ktap + kk] = X[a_off + m*a_pitch + tap*tap_stride + kk]
          const int tap = k / p.ktap;
          ra[i] = *reinterpret_cast<const f32x4*>(p.X + p.a_off + (int64_t)(m0 + row) * p.a_pitch +
                                                  (int64_t)tap * p.tap_stride + (k - tap * p.ktap));
        } else {
          ra[i] = *reinterpret_cast<const f32x4*>(p.X + (int64_t)(m0 + row) * p.ldx + k);
        }
      } else {
        const int m = m0 + row;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (m < p.M) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int kk = k + e;
            if (kk < p.K) {
              const int dr = kk / p.cin;
              v[e] = p.X[(int64_t)(m + dr) * p.ldx + (kk - dr * p.cin)];
            }
          }
        }
        ra[i] = v;
      }
    }
  };
  auto store_tiles = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = lr + 32 * i;
      *reinterpret_cast<f32x4*>(As + buf * TILE_F + row * LDT + c4 * 4) = ra[i];
      *reinterpret_cast<f32x4*>(Bs + buf * TILE_F + row * LDT + c4 * 4) = rb[i];
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  load_tiles(kt0);
  store_tiles(0);
  __syncthreads();

  const float* a_base = As + (wm * 64 + r32) * LDT + 4 * h;
  const float* b_base = Bs + (wn * 64 + r32) * LDT + 4 * h;

  for (int kt = kt0; kt < nk; ++kt) {
    const int cur = (kt - kt0) & 1;
    if (kt + 1 < nk) load_tiles(kt + 1);
    const float* ap = a_base + cur * TILE_F;
    const float* bp = b_base + cur * TILE_F;
#pragma unroll
    for (int q = 0; q < BK / 8; ++q) {
      f32x4 a0 = *reinterpret_cast<const f32x4*>(ap + q * 8);
      f32x4 a1 = *reinterpret_cast<const f32x4*>(ap + 32 * LDT + q * 8);
      f32x4 b0 = *reinterpret_cast<const f32x4*>(bp + q * 8);
      f32x4 b1 = *reinterpret_cast<const f32x4*>(bp + 32 * LDT + q * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // weights = MFMA A operand, activations = B operand: acc[ni][mi] is D[n][m] (xv_epilogue.h)
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b0[j], a0[j], acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b0[j], a1[j], acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b1[j], a0[j], acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b1[j], a1[j], acc[1][1], 0, 0, 0);
      }
    }
    if (kt + 1 < nk) store_tiles(cur ^ 1);
    __syncthreads();
  }

  // the final barrier of the K loop has retired every LDS read: reuse the tiles as store scratch
  store_wave_tile(p, acc, m0 + wm * 64, n0 + wn * 64, lane, wave, reinterpret_cast<char*>(smem));
}

// out[m][n] = act((sum_s partial[s][m][n]) * scale[n] + shift[n]); slices summed in index order.
__global__ void splitk_reduce_kernel(GemmArgs p) {
  const int64_t total = (int64_t)p.M * p.N;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int m = (int)(i / p.N), n = (int)(i - (int64_t)m * p.N);
    float acc = 0.f;
    for (int s = 0; s < p.ksplit; ++s) acc += p.partial[((int64_t)s * p.M + m) * p.Npad + n];
    bool zero;
    const int orow = out_row(p, m, zero);
    if (orow < 0) continue;
    float v = fmaf(acc, p.scale[n], p.shift[n]);
    if (p.R) v += p.R[(int64_t)orow * p.ldr + n];          // residual shortcut before the activation
    p.Y[(int64_t)orow * p.ldy + n] = zero ? 0.f : apply_act(v, p.act, p.alpha ? p.alpha[n] : 0.f);
  }
}

// ------------------------------------------------------------------------------ segment-level layers
// M <= 512 rows (one per utterance: tdnn6 / tdnn7, the extended TDNN's tdnn12, the ResNet's dense1/2, the attention post
// layers), dense, fp32 out.  The 128 x 128 kernel above gives such a layer 8 tiles, so it was run split-K over the chip with the
// partial sums going through HBM and a second launch adding them.  Here one launch does it: a workgroup owns a 32 x 16 output
// tile (256 x 512 -> 256 workgroups, one per CU), its eight waves take the 32-wide K steps round robin (step s -> wave s % 8)
// and the eight partial tiles are added in wave order through LDS before scale / shift / activation.  Deterministic: a fixed
// summation order.
//  * v_mfma_f32_16x16x4_f32 (same FLOP per clock as the 32x32x2 shape, exact products); weights = A operand, activations =
//    B operand, so a lane ends up with four consecutive channels of one row, as in xv_epilogue.h.
//  * No LDS in the K loop: lane (i, g) loads the eight consecutive k = 32 s + 8 g .. + 7 of row i straight from global
//    memory (two 16-byte loads per operand tile per eight MFMAs, a wave instruction pair = whole 128-byte lines of 16 rows; the K
//    index of an MFMA is only a summation label, so both operands use the same permuted order) and the loads run SG_PF steps
//    ahead of the MFMAs in a register ring.
//  * Consecutive workgroup ids walk the N tiles of one M tile: the ids congruent mod 8 (one XCD) then touch one eighth of the
//    weights each, and every XCD reads the activations once.
//  * 256 x 3000 x 512 takes it about 22 us, against 31 us for the pair it replaces (profiles/small_launches.md).  A ring half as
//    deep with 64-byte pieces per row took the same time and the MFMAs are 5 us of the whole chip, so the likely limit (inferred:
//    no fetch counters were taken) is the bytes a CU pulls through its L1 -- (32 + 16) rows x K x 4 = 577 KB per workgroup,
//    148 MB over the chip.  A 32 x 32 tile would move 98 MB on half the CUs; that form was not measured.
constexpr int SG_TM = 32, SG_TN = 16, SG_WAVES = 8, SG_KS = 32, SG_PF = 4;

__global__ __launch_bounds__(SG_WAVES * 64) void gemm_f32_seg_kernel(GemmArgs p, int nNt, int vec_out) {
  __shared__ __attribute__((aligned(16))) float red[SG_WAVES][SG_TM * SG_TN];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, g = lane >> 4;
  const int mt = blockIdx.x / nNt, nt = blockIdx.x - mt * nNt;
  const int m0 = mt * SG_TM, n0 = nt * SG_TN;
  const int nks = p.Kpad / SG_KS;

  // rows past M are computed on a copy of row M - 1 and never stored; the weights are zero padded to [Npad][Kpad]
  const float* wrow = p.Wt + (int64_t)(n0 + i16) * p.Kpad + 8 * g;
  const float* xrow0 = p.X + (int64_t)min(m0 + i16, p.M - 1) * p.ldx;
  const float* xrow1 = p.X + (int64_t)min(m0 + 16 + i16, p.M - 1) * p.ldx;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  // Every load is unconditional -- a step past the end re-reads the last one, a quad behind K (K % 4 == 0: it is inside the row
  // or behind it) the row's last quad -- and what must not count is zeroed when it is used: with the loads under a condition the
  // compiler put them behind branches and drained the whole ring (vmcnt(0)) once per trip, one memory latency per SG_PF steps.
  f32x4 rw[SG_PF][2], rx0[SG_PF][2], rx1[SG_PF][2];
  auto load_step = [&](int s, int i) {
    const int k = min(s, nks - 1) * SG_KS;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int kx = min(k + 8 * g + 4 * c, p.K - 4);
      rw[i][c] = *reinterpret_cast<const f32x4*>(wrow + k + 4 * c);
      rx0[i][c] = *reinterpret_cast<const f32x4*>(xrow0 + kx);
      rx1[i][c] = *reinterpret_cast<const f32x4*>(xrow1 + kx);
    }
  };
  // Compiler order only (no instruction): without it the loads of the ring are folded through the loop's phi nodes into one load
  // per slot at the top of the body, right in front of its use ...
  auto keep_here = [] {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);       // ... and the scheduler moved every load of a trip behind the trip's last MFMA
  };

  f32x4 acc0 = z, acc1 = z;
#pragma unroll
  for (int i = 0; i < SG_PF; ++i) load_step(wave + i * SG_WAVES, i);
  keep_here();
  for (int s = wave; s < nks; s += SG_PF * SG_WAVES) {
#pragma unroll
    for (int i = 0; i < SG_PF; ++i) {
      const int si = s + i * SG_WAVES;
      const bool in = si < nks;
      f32x4 w[2], x0[2], x1[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const bool inx = in && si * SG_KS + 8 * g + 4 * c < p.K;
        w[c] = in ? rw[i][c] : z;                    // (steps past the end add exact zeros)
        x0[c] = inx ? rx0[i][c] : z;
        x1[c] = inx ? rx1[i][c] : z;
      }
      load_step(si + SG_PF * SG_WAVES, i);
      keep_here();
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[c][j], x0[c][j], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[c][j], x1[c][j], acc1, 0, 0, 0);
        }
    }
  }

  // D[n][m]: lane (i16, g) holds channels 4 g .. 4 g + 3 of rows i16 and 16 + i16
  *reinterpret_cast<f32x4*>(&red[wave][i16 * SG_TN + 4 * g]) = acc0;
  *reinterpret_cast<f32x4*>(&red[wave][(16 + i16) * SG_TN + 4 * g]) = acc1;
  __syncthreads();
  if (tid >= SG_TM * SG_TN / 4) return;
  const int ml = tid >> 2, q = tid & 3;
  f32x4 acc = *reinterpret_cast<const f32x4*>(&red[0][ml * SG_TN + 4 * q]);
#pragma unroll
  for (int w = 1; w < SG_WAVES; ++w) acc += *reinterpret_cast<const f32x4*>(&red[w][ml * SG_TN + 4 * q]);
  const int m = m0 + ml, n = n0 + 4 * q;
  if (m >= p.M || n >= p.N) return;
  float* y = p.Y + (int64_t)m * p.ldy + n;
  if (vec_out) {                                   // N % 4 == 0: the whole quad is inside the row
    const f32x4 sc = *reinterpret_cast<const f32x4*>(p.scale + n), sh = *reinterpret_cast<const f32x4*>(p.shift + n);
    const f32x4 al = p.alpha ? *reinterpret_cast<const f32x4*>(p.alpha + n) : z;
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = apply_act(fmaf(acc[e], sc[e], sh[e]), p.act, al[e]);
    *reinterpret_cast<f32x4*>(y) = v;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (n + e < p.N) y[e] = apply_act(fmaf(acc[e], p.scale[n + e], p.shift[n + e]), p.act, p.alpha ? p.alpha[n + e] : 0.f);
  }
}

// true when gemm_f32_seg_kernel runs this launch
static bool seg_form(const GemmArgs& a, bool aligned) {
  return aligned && !a.a_pitch && a.M <= 512 && a.Y && !a.rowmap && !a.R && !a.Ysb && !a.pool_part && !a.att_part && !a.raw;
}

int gemm_f32_ksplit(int M, int Kpad, int Npad) {
  if (M > 512) return 1;                       // frame-level layers fill the chip on their own
  const int tiles = ((M + BM - 1) / BM) * (Npad / BN), nk = Kpad / BK;
  int s = 512 / (tiles > 0 ? tiles : 1);
  if (s > nk / 4) s = nk / 4;                  // at least four K tiles per slice
  return s < 2 ? 1 : s;
}

hipError_t launch_gemm_f32(const GemmArgs& a, bool aligned, hipStream_t s) {
  if (a.M <= 0) return hipSuccess;
  if (seg_form(a, aligned)) {
    // (The planner still reserves the split-K partials of such a layer -- a.partial, a.ksplit: the reservation is part of the
    // recorded plans -- but nothing is written there any more.)
    const int nMt = (a.M + SG_TM - 1) / SG_TM, nNt = (a.N + SG_TN - 1) / SG_TN;
    const int vec_out = (a.N & 3) == 0 && (a.ldy & 3) == 0 && (reinterpret_cast<uintptr_t>(a.Y) & 15) == 0 &&
                        (reinterpret_cast<uintptr_t>(a.scale) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.shift) & 15) == 0 &&
                        (reinterpret_cast<uintptr_t>(a.alpha) & 15) == 0;
    hipLaunchKernelGGL(gemm_f32_seg_kernel, dim3(nMt * nNt), dim3(SG_WAVES * 64), 0, s, a, nNt, vec_out);
    return hipGetLastError();
  }
  const int nMt = (a.M + BM - 1) / BM, nNt = a.Npad / BN;
  const int ks = (a.ksplit > 1 && a.partial && !a.Ysb && !a.pool_part) ? a.ksplit : 1;
  const int nk_all = a.Kpad / BK;
  const int kper = (nk_all + ks - 1) / ks;
  const size_t smem = (size_t)4 * TILE_F * sizeof(float);
  static std::mutex init_mu;    // per-device attributes; any thread may make the first launch on a device
  static bool attr_set[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  std::lock_guard<std::mutex> init_lock(init_mu);
  if (!attr_set[dev & 63]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_f32_kernel<2>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_f32_kernel<1>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_f32_kernel<0>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    attr_set[dev & 63] = true;
  }
  GemmArgs b = a;
  b.ksplit = ks;
  dim3 grid(nMt * nNt * ks), block(256);
  if (aligned && a.a_pitch)
    hipLaunchKernelGGL(gemm_f32_kernel<2>, grid, block, smem, s, b, nMt, nNt, kper);
  else if (aligned)
    hipLaunchKernelGGL(gemm_f32_kernel<1>, grid, block, smem, s, b, nMt, nNt, kper);
  else
    hipLaunchKernelGGL(gemm_f32_kernel<0>, grid, block, smem, s, b, nMt, nNt, kper);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || ks == 1) return e;
  const int64_t total = (int64_t)a.M * a.N;
  const int blocks = (int)((total + 255) / 256 > 1024 ? 1024 : (total + 255) / 256);
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, s, b);
  return hipGetLastError();
}

}  // namespace xv
