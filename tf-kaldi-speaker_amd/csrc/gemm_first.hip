// First TDNN layer (a convolution of w <= 5 taps over ONE 32-channel block: the 30-dim features staged as split-blocked rows)
// on workgroups that walk the M tiles with their weights resident.
//
// gemm_bf16x3_w14p2_kernel (gemm_bf16x3.hip) runs this layer as 128 x 128 tiles whose K loop is 5 steps long, so everything a
// 112-step convolution tile amortises is paid per tile: a prologue that drains the weight and slab loads, 80 KB of weight
// fragments per tile for a 320 KB matrix, the same slab staged by the four workgroups of an M tile, and a last, nearly empty
// round of the grid that cannot be K-split (one channel block).  Here
//   * the grid is two workgroups per CU, rounded down to a multiple of the N tiles; workgroup g owns N tile g % nNt for its
//     whole life and walks M tiles g / nNt, + grid / nNt, ... (static: no counter, no atomics, repeats are bit-identical);
//   * wave k owns 32-channel block k of the N tile, as in w14p2_tile, and keeps the weight fragments of taps 0..3 in registers
//     for the whole walk (64 VGPRs); the epilogues of xv_epilogue_n32.h / xv_f6.h are called unchanged;
//   * the slabs (136 rows, the rows and the swizzle of w14p2_tile: no byte is read that the tile kernel does not read) go
//     through two LDS buffers by global_load_lds_dwordx4.  The slab of the next tile is issued in front of the K loop of the
//     current one, into the buffer whose last fragment reads lie behind the workgroup barrier that closed the previous K loop;
//     it is waited for (s_waitcnt vmcnt(0), which the K loop has covered, then the barrier) between this K loop and its
//     epilogue, so neither the LDS-DMA latency nor the acknowledgement of the previous epilogue's stores is exposed;
//   * the epilogue scratch (4 x 8 KB) is its own LDS region: a slab is in flight or resident in both buffers while it is used;
//   * what an epilogue loads per tile -- the row map entries of its rows, BN scale and shift -- it finds in LDS: GemmArgs is
//     handed over with those three pointers set to LDS copies (the row map comes with the slab, by LDS-DMA).  Loads and stores
//     share one in-order counter, so a row map load behind the stores of the first 64-row pass waited for their
//     acknowledgement; that wait, not arithmetic, was most of an epilogue (the first version of this kernel, without the
//     copies, took 92 us where the tile kernel takes 81; with them 65: profiles/first_layer.md).
// The sums are those of k_step: per accumulator and tap, in tap order, hi * lo, lo * hi, then hi * hi -- the output is
// bit-identical to the tile kernel's.  The compiler schedules this file; there is no counted wait in it.
#include <mutex>

#include "xv_f6.h"

namespace xv {

namespace {
constexpr int BM = 128, BN = 128;
constexpr int DROW = 128;                          // unpadded LDS row
constexpr int DA_ROWS = 136;                       // 128 + (w - 1 <= 4) halo rows, multiple of 8
constexpr int DA_BYTES = DA_ROWS * DROW;
constexpr int MAXW = 5;                            // taps this kernel takes
// Taps whose weights stay in registers for the whole walk; tap 4 (16 VGPRs, 16 KB per workgroup from L2) is re-read per tile in front
// of the K loop and used last.  All five resident also compile without a spill (254 / 256 / 245 VGPRs against 239 / 247 / 235),
// and measured 3-5 us per forward slower than this on two machines (profiles/first_layer.md).
constexpr int RES = 4;
constexpr int EPI_BYTES = 4 * 64 * 128;            // epilogue scratch: 64 frames x 128 B per wave and pass
constexpr int RMAP_BYTES = 4 * 2 * BM * 4;         // row map entries of a tile: per wave its own copy, two buffers
constexpr int PAR_BYTES = 2 * BN * 4;              // BN scale and shift of the N tile
constexpr size_t SMEM_BYTES = (size_t)2 * DA_BYTES + EPI_BYTES + RMAP_BYTES + PAR_BYTES;      // 72 704 B: two workgroups per CU
typedef __attribute__((address_space(3))) void* lptr_t;
}  // namespace

// s_waitcnt vmcnt(0) as the builtin, not as inline assembly: the compiler's own wait insertion sees it, and so does not wait a second
// time -- for loads it believes pending -- in front of the first MFMA of a tile, where the LDS-DMA of the next slab and the previous
// epilogue's stores are in flight.  (gfx9 encoding: vmcnt 0, expcnt 7 and lgkmcnt 15 = no wait.)
__device__ __forceinline__ void wait_vm0() { __builtin_amdgcn_s_waitcnt(0x0F70); }

// EPI 0: activations (fp32 and / or split-blocked), EPI 3: the two-unit block format (fp16 only).
template <int EPI, bool F16>
__global__ __launch_bounds__(256, 2) void first_walk_kernel(GemmArgs p, int nMt, int nNt, int w) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* As = smem;
  char* scratch = smem + 2 * DA_BYTES;
  float* par = reinterpret_cast<float*>(smem + 2 * DA_BYTES + EPI_BYTES + RMAP_BYTES);      // scale[BN] | shift[BN]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c16 = lane & 15, g4 = lane >> 4;       // 16x16x32 operand maps: row / column lane & 15, k chunk lane >> 4

  const int nt = (int)blockIdx.x % nNt;
  const int mt_step = (int)gridDim.x / nNt;         // the grid is a multiple of nNt
  int mt = (int)blockIdx.x / nNt;
  if (mt >= nMt) return;                            // (the grid never exceeds the tile count: whole workgroup, before any barrier)
  const int n0 = nt * BN;

  const int ngroups = (BM + w - 1 + 7) >> 3;        // 8-row pieces of a slab
  const int lrow = lane >> 3, lpc = lane & 7;
  const int64_t a_row_bytes = p.ldsbx * 4;          // one 32-channel block per row: 128
  const char* Ag = reinterpret_cast<const char*>(p.Xsb) + (int64_t)lrow * a_row_bytes +
                   ((lpc ^ (((lrow >> 1) & 3) << 1)) << 4);      // slab swizzle on the source: chunk c at c ^ 2 * ((row >> 1) & 3)
  const uint32_t as_lds = (uint32_t)(uintptr_t)(lptr_t)As;
  int32_t* rmap = reinterpret_cast<int32_t*>(smem + 2 * DA_BYTES + EPI_BYTES) + wave * (2 * BM);
  auto dma_slab = [&](int m0, int buf) {
    for (int g = wave; g < ngroups; g += 4) {
      const char* src = Ag + (int64_t)(m0 + 8 * g) * a_row_bytes;
      const uint32_t dst = __builtin_amdgcn_readfirstlane(as_lds + buf * DA_BYTES + g * 1024);
      asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(dst) : "memory");
    }
    // The tile's 128 row map entries, into this wave's own copy (entry of row m0 + i at index i; rows from M on are never looked
    // at).  The epilogues read the row map and the BN vectors through GemmArgs: pointed at LDS they cost no vector-memory load, so
    // no wave waits inside an epilogue for the acknowledgement of the stores it issued before (loads and stores share vmcnt).
    int32_t* rm = rmap + buf * BM;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int32_t* src = p.rowmap + min(m0 + h * 64 + lane, p.M - 1);
      const uint32_t dst = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lptr_t)(rm + h * 64));
      asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" ::"v"(src), "s"(dst) : "memory");
    }
  };
  dma_slab(mt * BM, 0);

  // weight fragments of every tap: [tap][plane * 2 + channel tile], fragment-major (1 KB per wave and fragment)
  bf16x8 W[MAXW][4];
  const char* Wg = reinterpret_cast<const char*>(p.Wfr) + (int64_t)((n0 >> 5) + wave) * ((int64_t)(p.Kpad >> 5) * 4096) + lane * 16;
  auto load_w = [&](int j) __attribute__((always_inline)) {
    const char* q = Wg + (j < w ? j : 0) * 4096;      // (a tap the layer does not have: loaded from tap 0, never used)
#pragma unroll
    for (int f = 0; f < 4; ++f) W[j][f] = *reinterpret_cast<const bf16x8*>(q + f * 1024);
  };
#pragma unroll
  for (int j = 0; j < RES; ++j) load_w(j);
  if (tid < BN) {
    const int n = min(n0 + tid, p.N - 1);
    par[tid] = p.scale[n];
    par[BN + tid] = p.shift[n];
  }
  // what the epilogues see: rows relative to the tile (row map entry i = row m0 + i), BN vectors indexed by the absolute channel
  GemmArgs q = p;
  q.scale = par - n0;
  q.shift = par + BN - n0;
  wait_vm0();
  __syncthreads();

  for (int buf = 0; mt < nMt; mt += mt_step, buf ^= 1) {
    // next slab: the other buffer was last read in the previous K loop, behind that loop's closing barrier
    if (mt + mt_step < nMt) dma_slab((mt + mt_step) * BM, buf ^ 1);
#pragma unroll
    for (int j = RES; j < MAXW; ++j) load_w(j);
    int c16o = c16;                        // opaque: the per-tap fragment addresses are recomputed per tile, not kept across the epilogue
    asm volatile("" : "+v"(c16o));

    f32x4 acc[8][2];                       // [16-frame tile][16-channel tile]
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int c = 0; c < 2; ++c) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const char* slab = As + buf * DA_BYTES;
#pragma unroll
    for (int j = 0; j < MAXW; ++j) {
      if (j < w) {
        const char* ab = slab + (c16o + j) * DROW;
        const int aswz = (((c16o + j) >> 1) & 3) << 1;             // (16 ft + r) >> 1 == r >> 1 (mod 4)
        const int off_hi = (g4 ^ aswz) << 4, off_lo = ((4 + g4) ^ aswz) << 4;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
          const bf16x8 fh = *reinterpret_cast<const bf16x8*>(ab + off_hi + g * (16 * DROW));
          const bf16x8 fl = *reinterpret_cast<const bf16x8*>(ab + off_lo + g * (16 * DROW));
          acc[g][0] = mfma_split16<F16>(W[j][0], fl, acc[g][0]);
          acc[g][1] = mfma_split16<F16>(W[j][1], fl, acc[g][1]);
          acc[g][0] = mfma_split16<F16>(W[j][2], fh, acc[g][0]);
          acc[g][1] = mfma_split16<F16>(W[j][3], fh, acc[g][1]);
          acc[g][0] = mfma_split16<F16>(W[j][0], fh, acc[g][0]);
          acc[g][1] = mfma_split16<F16>(W[j][1], fh, acc[g][1]);
        }
      }
    }
    // the next slab has landed (every wave waits for its own pieces, then the barrier), and no wave reads this buffer again
    wait_vm0();
    __syncthreads();
    int lane_e = lane;                     // opaque: the epilogue's per-lane addresses are not hoisted over the walk
    asm volatile("" : "+v"(lane_e));
    const int m0 = mt * BM;
    q.rowmap = rmap + buf * BM;
    q.M = p.M - m0;
    if constexpr (EPI == 3) {
      // The block-format epilogue takes the activation at run time, and with it a conditional load of the PReLU slopes whose
      // destination registers the compiler guards with s_waitcnt vmcnt(0) on every path -- which also waits for the stores of the
      // pass before.  This instantiation is launched for ReLU only (launch_gemm_first): the activation is a constant of the
      // inlined copy here, as the ACT template argument of store_wave_tile_n32 is, and the load and its waits are gone.
      q.act = ACT_RELU;
      q.alpha = nullptr;
      store_wave_tile_n32_f6(q, acc, 0, n0 + wave * 32, lane_e, wave, scratch);
    } else {
      store_wave_tile_n32<F16>(q, acc, 0, n0 + wave * 32, lane_e, wave, scratch);
    }
  }
}

bool gemm_first_ok(const GemmArgs& a) {
  if (a.cin != 32 || a.ldsbx != 32 || a.K <= 0 || a.K % 32 != 0) return false;
  const int w = a.K / 32;
  if (w > MAXW || a.Kpad != a.K || a.Npad <= 0 || a.Npad % BN != 0 || a.M <= 0 || !a.Xsb || !a.Wfr) return false;
  if (!a.rowmap) return false;            // (every multi-tap layer has one; the kernel copies it to LDS tile by tile)
  if (a.a_pitch || a.arow || a.R || a.pool_part || a.att_part || a.pool_w || a.raw || a.tail_mt > 0) return false;
  // the block-format producer exists for 5 taps and in fp16, as in the tile kernel; here also for ReLU only (first_walk_kernel)
  if (a.ysb_f6) return a.f16 && w >= 5 && a.Ysb && !a.Y && a.act == ACT_RELU;
  return true;
}

hipError_t launch_gemm_first(const GemmArgs& a, hipStream_t s, bool* taken) {
  *taken = false;
  if (!gemm_first_ok(a)) return hipSuccess;
  static std::mutex init_mu;    // attributes and the CU count are per device; any thread may make the first launch on one
  static int cus_of[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  int cus;
  {
    std::lock_guard<std::mutex> init_lock(init_mu);
    if (!cus_of[dev & 63]) {
      const void* kernels[] = {reinterpret_cast<const void*>(first_walk_kernel<3, true>), reinterpret_cast<const void*>(first_walk_kernel<0, true>),
                               reinterpret_cast<const void*>(first_walk_kernel<0, false>)};
      for (const void* k : kernels) {
        const hipError_t r = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SMEM_BYTES);
        if (r != hipSuccess) return r;
      }
      int n = 0;
      if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
      cus_of[dev & 63] = n;
    }
    cus = cus_of[dev & 63];
  }
  const int w = a.K / 32;
  const int nNt = a.Npad / BN, nMt = (a.M + BM - 1) / BM;
  int64_t grid = (int64_t)2 * cus;                           // two workgroups per CU (register and LDS budget)
  if (grid > (int64_t)nMt * nNt) grid = (int64_t)nMt * nNt;
  grid -= grid % nNt;
  if (grid <= 0) return hipSuccess;                          // more N tiles than workgroup slots: the tile kernel
  const dim3 g((unsigned)grid), block(256);
  if (a.ysb_f6) hipLaunchKernelGGL((first_walk_kernel<3, true>), g, block, SMEM_BYTES, s, a, nMt, nNt, w);
  else if (a.f16) hipLaunchKernelGGL((first_walk_kernel<0, true>), g, block, SMEM_BYTES, s, a, nMt, nNt, w);
  else hipLaunchKernelGGL((first_walk_kernel<0, false>), g, block, SMEM_BYTES, s, a, nMt, nNt, w);
  *taken = true;
  return hipGetLastError();
}

}  // namespace xv
