// bf16x3 split-precision MFMA GEMM for gfx950 (MI355X): the TDNN's temporal convolutions and
// dense layers at ~fp32 accuracy on the bf16 matrix pipe.
//
//   x = hi + lo (+ O(2^-17 |x|)),  hi = rn_bf16(x), lo = rn_bf16(x - hi)
//   a*b ~= a_hi*b_hi + a_hi*b_lo + a_lo*b_hi          (dropped terms ~2^-17 |a b|)
//
// Three v_mfma_f32_16x16x32_bf16 (or _f16: XV_PREC_F16X3) per product tile, fp32 accumulate: 16/3 = 5.3x the rate of
// the exact v_mfma_f32_32x32x2_f32 path at a relative error of ~5e-6 per layer (measured in
// tests/test_gpu_parity.py against the float64 oracle; the bar is 1e-4).
//
// Both operands arrive in the split-blocked format of xv_common.h: per row, 128-byte blocks
// [32 x bf16 hi | 32 x bf16 lo].  One block is one K step of 32 for one row, so
//   * every global access is a full 128-byte line (8 lanes x 16 bytes),
//   * 16-byte chunk q of a block is exactly a lane's MFMA fragment: plane q>>2 (hi / lo), k chunk q&3 = lane>>4 of
//     the 16x16x32 shape (k16-step (q>>1)&1, lane-half q&1 of 32x32x16) -- one ds_read_b128 per fragment, no repacking,
//   * a temporal convolution stays an "overlapping-row" GEMM: row m of A is the contiguous
//     run of w*cin/32 blocks that starts at frame m.
//
// The product kernels, on 128x128 workgroup tiles of 256 threads:
//   gemm_bf16x3_w14p2_kernel  multi-tap convolutions: activation slabs by LDS-DMA (two buffers, one slab per channel
//                             block), weight fragments straight into registers two steps ahead, one wave per
//                             32-channel block, counted waits; the K-split slices of the tail tiles ride in the same launch;
//   gemm_bf16x3_w1p3_kernel   one-tap layers (dense, attention epilogues, ResNet grid convolutions incl. the gathered
//                             compact-row form): three slab buffers, slabs two steps ahead.
#include <cstdlib>
#include <mutex>

#include "xv_f6.h"

namespace xv {

namespace {
constexpr int BM = 128, BN = 128;
constexpr int DROW = 128;                          // unpadded LDS row
constexpr int DA_ROWS = 136;                       // 128 + (w-1 <= 8) halo rows, multiple of 8
constexpr int DA_BYTES = DA_ROWS * DROW;
typedef __attribute__((address_space(3))) void* lptr_t;
}  // namespace

// ------------------------------------------------------------------------------------------
// Default kernel: 128x128 workgroup tile, "weights in registers", 1 x 4 wave layout, counted waits.
//
// How it got here (each step measured on MI355X, profiles/README.md; the intermediate kernels are in the git
// history: 3fd7543 weights in registers 2 x 2 waves, 659ee67 counted waits, c74e274 1 x 4 waves; d876abd is the last
// commit with the two first kernels, both operands by LDS-DMA / register-staged with one barrier per K step):
//  * the activation slab (frames [m0, m0 + 128 + w - 1) of one 32-channel block) goes global -> LDS with
//    global_load_lds_dwordx4: no VGPR staging, unpadded 128-byte rows made conflict-free by an XOR swizzle of the per-lane
//    SOURCE address and of the fragment read address, and all w taps of a convolution read the one slab by shifting the
//    fragment row (traffic / w).  The weight fragments never touch
//    LDS: they are packed a second time in MFMA-fragment-major order (one global_load_dwordx4 of a wave = 1 KB
//    contiguous; reading the row-major SB rows directly touches 32 lines per instruction and is 60 % slower) and
//    every lane loads its own fragments straight from L2 into VGPR buffers.  85 % of the LDS-DMA pieces of the
//    all-DMA kernel were weight tiles; they and their landing wait go, and the only LDS hazard left is the slab,
//    so the workgroup barrier drops from one per K step to one per channel block (every w steps);
//  * the epilogue scratch is 8 KB per wave (64 frames x 128 B per pass), the workgroup needs only the 34 KB of
//    the slabs, and THREE workgroups share a CU (12 waves);
//  * every wave owns ONE 32-channel block and all 128 frames of the tile.  With 2 x 2 waves the two waves of a
//    pair load identical weight fragments; the L1 counters showed the second request landing on a line still in
//    flight 36 % of all L1 cycles (TCP_PENDING_STALL_CYCLES, profiles/r01/pmc_tcp1_wreg.txt) and the texture
//    addresser busy 62 % of the kernel.  Here every weight byte is requested once per workgroup (4 loads per
//    wave and step); the price is that all four waves read the whole slab from LDS (16 ds_read_b128 per wave and
//    step), which the LDS has room for (halving the LDS reads of the 2 x 2 kernel changed nothing);
//  * every vector-memory instruction of the K loop is inline assembly, issued one per group of 3 MFMAs in the
//    order the fragments are needed (a burst from all waves of the CU queues up in the texture addresser and the
//    in-order waves stop feeding the matrix pipe: -4..7 %), and every wait is an explicit s_waitcnt vmcnt(N) with
//    an exact count.  The compiler can only drain the counter (vmcnt(0)) when LDS-DMA and register loads are
//    mixed, and it needs the issue to be unconditional (a path that skips a load forces vmcnt(0)), hence the
//    clamped duplicate slab pieces instead of branches (NPS pieces per wave and step: 1 when w >= 5, else 4).
//    The counts rely on LDS-DMA loads and register loads retiring in issue order under the one counter (checked
//    on hardware: tools/vmcnt_order_test.hip, 0 violations in 2.6e8 trials).  The waits name the registers they
//    release as "+v" operands, so the compiler cannot move an MFMA above its wait.
#define XV_GLD(dst, ptr, OFF) asm volatile("global_load_dwordx4 %0, %1, off offset:" #OFF : "=v"(dst) : "v"(ptr))
#define XV_WAIT4(N, ra, rb, rc, rd) asm volatile("s_waitcnt vmcnt(%4)" : "+v"(ra), "+v"(rb), "+v"(rc), "+v"(rd) : "n"(N))

//  * the weight fragments are prefetched TWO steps ahead (three register buffers of 4 fragments).
//    With one step of lead a workgroup alone on a CU is bound by the load->use latency (~0.9 us per step against
// 0.4 us of MFMA work), so only three resident workgroups together cover the matrix pipe and every prologue,
// epilogue and the tail of the launch leave it under-fed; with two steps of lead two workgroups suffice.
//   VMEM order per step:  D x NPS (top) , a0 (group 0) a1 (group 2) a2 (group 4) a3 (group 6)   [for step s+2]
//   before the first MFMA of step s: vmcnt(5+2*NPS) [a0..a3 of step s, issued during step s-2: younger are the NPS slab
//   pieces + 4 weight loads of step s-1 and the NPS pieces + a0 of step s]; slab switch vmcnt(4).
//  * MFMA shape v_mfma_f32_16x16x32 (round 2): the wave tile is 8 x 2 accumulator tiles of 16 frames x 16 channels; per K
//    step 48 MFMAs of 16 cycles instead of 24 of 32 -- the same operand bytes, LDS reads and FLOP per cycle, but the chip
//    holds a clearly higher clock on this shape (a timing-only swap of the instruction inside this kernel: tdnn3_conv
//    0.591 -> 0.500 ms; profiles/README.md).
//  * K-split slices: the tile function takes the channel-block range [cb_begin, cb_end) so that the tail form
//    (gemm_bf16x3_tail_plan) can run one slice of K per workgroup.
// The activation fragment addresses use ONE swizzle and ONE row offset per lane ((32*mi + r) >> 1 == r >> 1 mod 8)
// plus ds_read immediates, which frees the registers for the third weight buffer at 3 workgroups / CU.
// EPI selects the epilogue at compile time: 0 = activations (fp32 / SB / residual / fused statistics pooling),
// 1 / 2 = the attention forms of xv_epilogue_n32.h (score partials of the last key layer / weighted moments of the value).
// A separate instantiation keeps the default kernel's code -- and its register allocation -- untouched.
// F16 selects the split format of both operands (bf16 hi/lo or fp16 hi/lo: same bytes, same MFMA rate).

// workgroup -> (M tile, N tile).  Product order: ids congruent mod 8 share an XCD; an XCD owns a contiguous run of
// tiles, N fastest, so the nNt workgroups that stage the same slab start together on the same L2.
__device__ __forceinline__ void tile_of_block(int id, int nMt, int nNt, int& mt, int& nt) {
  const int tile = xcd_remap(id, nMt * nNt);
  mt = tile / nNt;
  nt = tile - mt * nNt;
}

// ---- what the two tile functions below share ----
// (Their accumulator clear and their epilogue dispatch on EPI stay written out in both: as helpers they changed the emitted
// code of the kernels, tools/isa_same.py.)
// One K step of a wave: 8 frame tiles x 2 channel tiles x (hi*lo, lo*hi, hi*hi) on the weights Wc, while the weights of
// step s + 2 are loaded from q into Wn.  `ab` is this lane's row of the current slab, off_hi / off_lo its k chunk of the
// hi / lo half behind the slab swizzle; issue_slab() issues the step's slab pieces (unconditionally, see above); WAITN is
// the vmcnt at which Wc, issued two steps earlier, has landed (counted in front of each tile function).
// Slab swizzle (w14p2): chunk c of slab row r lives at position c ^ 2 * ((r >> 1) & 3).  A ds_read_b128 is served in groups of 16
// lanes = 16 consecutive rows of which the outer eight read k chunk g4 and the inner eight g4 ^ 1 (lane groups of the
// instruction: MI355X_MICROARCH.md, LDS); with the tap shift j the window starts at any row, and only a swizzle that leaves
// bit 0 of the chunk alone keeps those two sets apart for every start (the round-2 swizzle (r >> 1) & 7, which the one-tap
// form keeps, was conflict-free for j = 0 mod 4 only: tests/analysis/lds_bank_model.py, SQ_LDS_BANK_CONFLICT).
template <bool F16, int WAITN, class IssueSlab>
__device__ __forceinline__ void k_step(f32x4 (&acc)[8][2], bf16x8 (&Wc)[4], bf16x8 (&Wn)[4], const char* q, const char* ab,
                                       int off_hi, int off_lo, IssueSlab issue_slab) {
  bf16x8 fh[8], fl[8];                   // activation fragments of frame tile ft, read two tiles ahead
  auto read_frag = [&](int ft) {
    fh[ft] = *reinterpret_cast<const bf16x8*>(ab + off_hi + ft * (16 * DROW));
    fl[ft] = *reinterpret_cast<const bf16x8*>(ab + off_lo + ft * (16 * DROW));
  };
  read_frag(0);
  read_frag(1);
  issue_slab();
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int g = 0; g < 8; ++g) {          // g = frame tile: 6 MFMAs of 16 cycles
    if (g == 0) XV_GLD(Wn[0], q, 0);          // hi, channels 0..15
    if (g == 2) XV_GLD(Wn[1], q, 1024);       // hi, channels 16..31
    if (g == 4) XV_GLD(Wn[2], q, 2048);       // lo, channels 0..15
    if (g == 6) XV_GLD(Wn[3], q, 3072);       // lo, channels 16..31
    if (g + 2 < 8) read_frag(g + 2);
    if (g == 0) XV_WAIT4(WAITN, Wc[0], Wc[1], Wc[2], Wc[3]);
    // small cross terms first, the dominant hi*hi term last; the two channel tiles alternate
    acc[g][0] = mfma_split16<F16>(Wc[0], fl[g], acc[g][0]);
    acc[g][1] = mfma_split16<F16>(Wc[1], fl[g], acc[g][1]);
    acc[g][0] = mfma_split16<F16>(Wc[2], fh[g], acc[g][0]);
    acc[g][1] = mfma_split16<F16>(Wc[3], fh[g], acc[g][1]);
    acc[g][0] = mfma_split16<F16>(Wc[0], fh[g], acc[g][0]);
    acc[g][1] = mfma_split16<F16>(Wc[1], fh[g], acc[g][1]);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// End of the K loop.  Every wave's last (dummy) slab pieces have landed before any wave turns the slab buffers into its
// epilogue scratch: the waves of a workgroup can be a step apart here, and a piece issued at the top of that step may still
// be in flight.  Returns the lane id made opaque: the epilogue's per-lane addresses all derive from it, and so they cannot be
// hoisted above the K loop, where they would cost registers (and spill) for its whole duration.
__device__ __forceinline__ int end_k_loop(const GemmArgs& p, int lane) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  __builtin_amdgcn_sched_barrier(0);
  XV_EPI_STAMP(p, 2);
  asm volatile("" : "+v"(lane));
  return lane;
}

template <int NPS, int EPI = 0, bool F16 = false>
__device__ __forceinline__ void w14p2_tile(const GemmArgs& p, int m0, int n0, int w, char* smem3, int cb_begin, int cb_end, bool slice = false) {
  char* As = smem3;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c16 = lane & 15, g4 = lane >> 4;       // 16x16x32 operand maps: row / column lane & 15, k chunk lane >> 4

  const int ncb = (p.Kpad >> 5) / w;
  const int nsteps = (cb_end - cb_begin) * w;      // channel blocks [cb_begin, cb_end): the whole K, or one K-split slice
  const int ngroups = (BM + w - 1 + 7) >> 3;
  const int lrow = lane >> 3, lpc = lane & 7;
  const int64_t a_row_bytes = (p.a_pitch ? p.a_pitch : p.ldsbx) * 4;
  const int kbt = p.a_pitch ? (p.ktap >> 5) : (p.Kpad >> 5);
  const int64_t tap_bytes = p.a_pitch ? p.tap_stride * 4 : 0;
  const char* Ag = reinterpret_cast<const char*>(p.Xsb) + p.a_off * 4 + (int64_t)(m0 + lrow) * a_row_bytes;
  const int64_t nkb4k = (int64_t)(p.Kpad >> 5) * 4096;
  const char* Wg = reinterpret_cast<const char*>(p.Wfr) + (int64_t)((n0 >> 5) + wave) * nkb4k + lane * 16;
  const uint32_t as_lds = (uint32_t)(uintptr_t)(lptr_t)As;

  auto dma_a = [&](int64_t koff, int buf, int g) {
    const int c = lpc ^ (((lrow >> 1) & 3) << 1);          // slab swizzle (k_step): 2 * ((row >> 1) & 3), row = 8 g + lrow
    const char* src = Ag + (int64_t)(8 * g) * a_row_bytes + koff + c * 16;
    const uint32_t dst = __builtin_amdgcn_readfirstlane(as_lds + buf * DA_BYTES + g * 1024);
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(dst) : "memory");
  };

  f32x4 acc[8][2];                       // [16-frame tile][16-channel tile]
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int c = 0; c < 2; ++c) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  // (cb, j) of the current step, of the next one and of the one after
  int cb = cb_begin, j = 0, cb1 = cb_begin, j1 = 1, cb2, j2;
  if (j1 == w) { j1 = 0; cb1 = cb_begin + 1; }
  cb2 = cb1; j2 = j1 + 1;
  if (j2 == w) { j2 = 0; cb2 = cb1 + 1; }

  XV_EPI_STAMP(p, 0);
  bf16x8 W0[4], W1[4], W2[4];            // [plane * 2 + channel tile]; W0: step 0, W1: step 1
  {
    const char* q1 = Wg + (int64_t)(1 < nsteps ? j1 * ncb + cb1 : 0) * 4096;
    const char* q0 = Wg + (int64_t)cb_begin * 4096;               // step 0 = (cb_begin, tap 0)
    XV_GLD(W0[0], q0, 0); XV_GLD(W0[1], q0, 1024); XV_GLD(W0[2], q0, 2048); XV_GLD(W0[3], q0, 3072);
    XV_GLD(W1[0], q1, 0); XV_GLD(W1[1], q1, 1024); XV_GLD(W1[2], q1, 2048); XV_GLD(W1[3], q1, 3072);
  }
  // (a K-split slice starts at block cb_begin of the row; slices exist in the 1-D form only)
  for (int g = wave; g < ngroups; g += 4) dma_a((int64_t)cb_begin * 128, cb_begin & 1, g);
  int64_t koff_next = (kbt == 1 && p.a_pitch) ? tap_bytes : (int64_t)(cb_begin + 1) * 128;
  int blk_next = (kbt == 1 && p.a_pitch) ? 0 : 1;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  XV_EPI_STAMP(p, 1);
  auto step = [&](int s, bf16x8 (&Wc)[4], bf16x8 (&Wn)[4]) __attribute__((always_inline)) {
    const int kbn = s + 2 < nsteps ? j2 * ncb + cb2 : 0;        // weights of step s + 2 (unconditional issue)
    const char* q = Wg + (int64_t)kbn * 4096;
    const char* ab = As + (cb & 1) * DA_BYTES + (c16 + j) * DROW;
    const int aswz = (((c16 + j) >> 1) & 3) << 1;               // slab swizzle (k_step): (16 ft + r) >> 1 == r >> 1 (mod 4)
    const int off_hi = (g4 ^ aswz) << 4, off_lo = ((4 + g4) ^ aswz) << 4;     // this lane's k chunk of the hi / lo half
    k_step<F16, 5 + 2 * NPS>(acc, Wc, Wn, q, ab, off_hi, off_lo, [&]() __attribute__((always_inline)) {
      const int64_t ksrc = cb + 1 < cb_end ? koff_next : 0;
#pragma unroll
      for (int i = 0; i < NPS; ++i) dma_a(ksrc, (cb + 1) & 1, min((j * NPS + i) * 4 + wave, ngroups - 1));
    });
    if (cb1 != cb) {                     // slab switch
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      __syncthreads();
      if (++blk_next == kbt) {
        blk_next = 0;
        koff_next += tap_bytes - (int64_t)(kbt - 1) * 128;
      } else {
        koff_next += 128;
      }
    }
    cb = cb1; j = j1;
    cb1 = cb2; j1 = j2;
    if (++j2 == w) { j2 = 0; ++cb2; }
  };
  for (int s = 0; s < nsteps; s += 3) {
    step(s, W0, W2);
    if (s + 1 < nsteps) step(s + 1, W1, W0);
    if (s + 2 < nsteps) step(s + 2, W2, W1);
  }
  const int lane_e = end_k_loop(p, lane);
  if constexpr (EPI == 3) {
    if (slice) {
      // K-split slice of a tail tile: the raw accumulators go to the slice's rows of GemmArgs::partial (p.Y / p.ldy were pointed
      // there by the kernel), 16-byte stores straight from the accumulator layout as in gemm_f6v2.hip -- a second LDS epilogue in
      // this instantiation would not fit its registers
      const int c16e = lane_e & 15, g4e = lane_e >> 4;
#pragma unroll
      for (int g = 0; g < 8; ++g)
#pragma unroll
        for (int c = 0; c < 2; ++c)
          *reinterpret_cast<f32x4*>(p.Y + (int64_t)(m0 + 16 * g + c16e) * p.ldy + n0 + wave * 32 + 16 * c + 4 * g4e) = acc[g][c];
      return;
    }
    store_wave_tile_n32_f6(p, acc, m0, n0 + wave * 32, lane_e, wave, smem3);      // XV_PREC_F16F6 producer: the two-unit block format
  } else if constexpr (EPI != 0) store_wave_tile_n32_att<EPI>(p, acc, m0, n0 + wave * 32, lane_e, wave, smem3);
  else store_wave_tile_n32<F16>(p, acc, m0, n0 + wave * 32, lane_e, wave, smem3);
  XV_EPI_STAMP(p, 3);
}

// One-tap form (dense layers, and the ResNet grid convolutions whose taps are plain K blocks): every K step needs a new
// activation slab.  With two slab buffers the slab of step s + 1 is issued at the top of step s and has to land within
// that one step (the wait at the end of the step exposes whatever is left of its ~1 us LDS-DMA latency, every step):
// measured 1.46-1.75 us per step against 1.36 us for the 7-tap convolution, whose slab has seven steps to land.  Here the
// slabs rotate through THREE buffers (52 KB of LDS, still three workgroups per CU) and are issued TWO steps ahead, like
// the weights; the wait at the end of step s only has to retire slab s + 1, issued a whole step earlier:
//   VMEM order per step:  D x 4 (slab s+2, top) , a0 a1 a2 a3 (weights s+2)
//   before the first MFMA: vmcnt(13) [younger than the weights of step s: slab s+1 (4), weights s+1 (4), slab s+2 (4),
//   the first weight load of s+2 (1)]; end of step: vmcnt(12)
//   [younger than slab s+1: weights s+1 (4), slab s+2 (4), weights s+2 (4)], then the workgroup barrier (RAW for the slab
//   read in step s+1; WAR for buffer (s+3) % 3 = s % 3, refilled at the top of step s+1).
// The loop is unrolled by three, so the slab buffer of a step is a compile-time constant like its weight registers.
template <int EPI, bool F16, bool GATHER = false>
__device__ __forceinline__ void w1p3_tile(const GemmArgs& p, int m0, int n0, char* smem3) {
  char* As = smem3;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c16 = lane & 15, g4 = lane >> 4;       // 16x16x32 operand maps: row / column lane & 15, k chunk lane >> 4

  const int nsteps = p.Kpad >> 5;
  const int lrow = lane >> 3, lpc = lane & 7;
  const int64_t a_row_bytes = (p.a_pitch ? p.a_pitch : p.ldsbx) * 4;
  const int kbt = p.a_pitch ? (p.ktap >> 5) : (p.Kpad >> 5);
  const int64_t tap_bytes = p.a_pitch ? p.tap_stride * 4 : 0;
  const char* Ag = reinterpret_cast<const char*>(p.Xsb) + p.a_off * 4 + (int64_t)(m0 + lrow) * a_row_bytes;
  const int64_t nkb4k = (int64_t)(p.Kpad >> 5) * 4096;
  // Channel-block role of this wave.  A layer narrower than the tile (ResNet stage 1: 64 channels in a 128-channel tile)
  // leaves two of the four blocks pure padding: the waves that own them only stage their share of the slabs and keep the
  // barriers (no weight loads, no MFMAs, no epilogue), and WHICH waves those are alternates with the workgroup's dispatch
  // slot, so that the computing waves of the workgroups sharing a CU do not all sit on the same two SIMDs.
  const bool narrow = EPI == 0 && p.N <= 64 && !p.pool_part && !p.raw;
  const int wv = narrow ? (wave ^ (((blockIdx.x >> 8) & 1) << 1)) : wave;
  const bool passive = narrow && n0 + wv * 32 >= p.N;
  const char* Wg = reinterpret_cast<const char*>(p.Wfr) + (int64_t)((n0 >> 5) + wv) * nkb4k + lane * 16;
  const uint32_t as_lds = (uint32_t)(uintptr_t)(lptr_t)As;

  // gathered form: this lane's four slab rows (groups wave, 4 + wave, 8 + wave, 12 + wave) start at grid positions
  // arow[...]; their byte offsets from the operand base (swizzled chunk included: (4 g) & 7 does not depend on i) stay in
  // four registers and every DMA is base (scalar, advanced with the K block) + offset (vector)
  uint32_t goff[4] = {0, 0, 0, 0};
  const char* gbase = reinterpret_cast<const char*>(p.Xsb) + p.a_off * 4;
  if constexpr (GATHER) {
    const int cg = lpc ^ ((4 * wave + (lrow >> 1)) & 7);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      goff[i] = (uint32_t)p.arow[m0 + lrow + 8 * (4 * i + wave)] * (uint32_t)a_row_bytes + cg * 16;
  }
  auto dma_a = [&](int64_t koff, int buf, int g) {
    const int c = lpc ^ ((4 * g + (lrow >> 1)) & 7);
    const char* src = Ag + (int64_t)(8 * g) * a_row_bytes + koff + c * 16;
    const uint32_t dst = __builtin_amdgcn_readfirstlane(as_lds + buf * DA_BYTES + g * 1024);
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(dst) : "memory");
  };
  auto dma_g = [&](const char* kbase, int buf, int i) {
    const uint32_t dst = __builtin_amdgcn_readfirstlane(as_lds + buf * DA_BYTES + (4 * i + wave) * 1024);
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(goff[i]), "s"(kbase), "s"(dst) : "memory");
  };
  auto dma_slab = [&](int64_t koff, int buf) {      // the 16 eight-row groups of a slab: four per wave
    if constexpr (GATHER) {
      const char* kbase = gbase + koff;
#pragma unroll
      for (int i = 0; i < 4; ++i) dma_g(kbase, buf, i);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) dma_a(koff, buf, i * 4 + wave);
    }
  };

  f32x4 acc[8][2];                       // [16-frame tile][16-channel tile]
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int c = 0; c < 2; ++c) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  XV_EPI_STAMP(p, 0);
  // byte offset inside an A row of the K block of the slab to issue next (1-D form: block * 128; grid form: tap * tap_bytes
  // + block-in-tap * 128), advanced incrementally
  int64_t koff_issue = 0;
  int blk_issue = 0;
  auto advance = [&]() {
    if (++blk_issue == kbt) {
      blk_issue = 0;
      koff_issue += tap_bytes - (int64_t)(kbt - 1) * 128;
    } else {
      koff_issue += 128;
    }
  };
  if (passive) {                          // uniform per wave: slabs and barriers only (see `narrow` above)
    dma_slab(0, 0);
    advance();
    dma_slab(1 < nsteps ? koff_issue : 0, 1);
    advance();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int s = 0, buf = 2; s < nsteps; ++s) {
      dma_slab(s + 2 < nsteps ? koff_issue : 0, buf);        // slab s + 2 into buffer (s + 2) % 3
      buf = buf == 2 ? 0 : buf + 1;
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");       // this wave's pieces of slab s + 1 have landed
      __syncthreads();
      advance();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                      // the barrier in front of the other waves' epilogue (below)
    return;
  }
  bf16x8 W0[4], W1[4], W2[4];            // [plane * 2 + channel tile]; W0: step 0, W1: step 1
  {
    const char* q0 = Wg;
    const char* q1 = Wg + (int64_t)(1 < nsteps ? 1 : 0) * 4096;
    XV_GLD(W0[0], q0, 0); XV_GLD(W0[1], q0, 1024); XV_GLD(W0[2], q0, 2048); XV_GLD(W0[3], q0, 3072);
    XV_GLD(W1[0], q1, 0); XV_GLD(W1[1], q1, 1024); XV_GLD(W1[2], q1, 2048); XV_GLD(W1[3], q1, 3072);
  }
  dma_slab(0, 0);                        // slab 0
  advance();
  dma_slab(1 < nsteps ? koff_issue : 0, 1);          // slab 1 (a duplicate of slab 0 when K is a single block)
  advance();                             // koff_issue now describes slab 2
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  XV_EPI_STAMP(p, 1);
  const int aswz = (c16 >> 1) & 7;       // (16 ft + r) >> 1 == r >> 1 (mod 8): one swizzle for all eight tiles
  const int off_hi = (g4 ^ aswz) << 4, off_lo = ((4 + g4) ^ aswz) << 4;       // this lane's k chunk of the hi / lo half
  auto step = [&](int s, int buf, bf16x8 (&Wc)[4], bf16x8 (&Wn)[4]) __attribute__((always_inline)) {
    const char* q = Wg + (int64_t)(s + 2 < nsteps ? s + 2 : 0) * 4096;      // weights of step s + 2 (unconditional issue)
    const char* ab = As + buf * DA_BYTES + c16 * DROW;
    k_step<F16, 13>(acc, Wc, Wn, q, ab, off_hi, off_lo, [&]() __attribute__((always_inline)) {
      dma_slab(s + 2 < nsteps ? koff_issue : 0, buf == 0 ? 2 : buf - 1);    // slab s + 2 into buffer (s + 2) % 3
    });
    asm volatile("s_waitcnt vmcnt(12)" ::: "memory");      // slab s + 1 has landed (this wave's pieces)
    __syncthreads();
    advance();
  };
  for (int s = 0; s < nsteps; s += 3) {
    step(s, 0, W0, W2);
    if (s + 1 < nsteps) step(s + 1, 1, W1, W0);
    if (s + 2 < nsteps) step(s + 2, 2, W2, W1);
  }
  const int lane_e = end_k_loop(p, lane);
  if constexpr (EPI == 3) store_wave_tile_n32_f6(p, acc, m0, n0 + wave * 32, lane_e, wave, smem3);      // XV_PREC_F16F6 producer
  else if constexpr (EPI != 0) store_wave_tile_n32_att<EPI>(p, acc, m0, n0 + wave * 32, lane_e, wave, smem3);
  else store_wave_tile_n32<F16>(p, acc, m0, n0 + wv * 32, lane_e, wave, smem3);      // wv: the block this wave computed (`narrow`)
  XV_EPI_STAMP(p, 3);
}

template <int EPI = 0, bool F16 = false, bool GATHER = false>
__global__ __launch_bounds__(256, 3) void gemm_bf16x3_w1p3_kernel(GemmArgs p, int nMt, int nNt) {
  extern __shared__ __attribute__((aligned(16))) char smem3[];
  int mt, nt;
  tile_of_block(blockIdx.x, nMt, nNt, mt, nt);
  w1p3_tile<EPI, F16, GATHER>(p, mt * BM, nt * BN, smem3);
}

// Workgroups [0, nMt * nNt) are whole tiles.  With S > 0 the grid continues with the K-split slices of the tail tiles
// (gemm_bf16x3_tail_plan: the M tiles nMt .. nMt + tail_mt - 1 of the last, nearly empty round): workgroup = (tile, slice),
// slice s accumulates channel blocks [s * ncb / S, (s + 1) * ncb / S) and stores its RAW accumulators to
// partial[s][row - nMt * 128][Npad]; bf16x3_tail_reduce_kernel adds the slices in order and runs the epilogue.  The slices
// are the highest workgroup ids, so they are dispatched into the slots the last whole tiles leave free -- as their own
// launch they ran latency-bound on an otherwise idle chip (17-21 us per layer for 1.4 % of its MFMA work).
template <int NPS, int EPI = 0, bool F16 = false>
__global__ __launch_bounds__(256, 3) void gemm_bf16x3_w14p2_kernel(GemmArgs p, int nMt, int nNt, int w, int S) {
  extern __shared__ __attribute__((aligned(16))) char smem3[];
  int mt, nt, cb_begin = 0, cb_end = (p.Kpad >> 5) / w;
  constexpr bool kSlices = EPI == 0 || EPI == 3;      // the attention forms are never K-split
  const bool slice = kSlices && (int)blockIdx.x >= nMt * nNt;
  if (slice) {
    const int id = blockIdx.x - nMt * nNt;
    const int split = id % S, tile = id / S;
    mt = nMt + tile / nNt;
    nt = tile % nNt;
    const int per = cb_end / S;
    cb_begin = split * per;
    cb_end = cb_begin + per;
    p.Y = p.partial + ((int64_t)split * p.tail_mt - nMt) * (int64_t)BM * p.Npad;   // row m of the tile -> slice row m - nMt*128
    p.ldy = p.Npad;
    if (EPI == 0) {                        // through the usual epilogue as raw sums (EPI == 3: the tile function's own raw store)
      p.raw = 1;
      p.act = ACT_NONE;                    // no scale / shift / activation before the reduce
      p.alpha = nullptr;
      p.N = p.Npad;
      p.M = (nMt + p.tail_mt) * BM;        // every row of the tail tiles is stored (rows >= M are never read back)
      p.Ysb = nullptr;
      p.rowmap = nullptr;
      p.R = nullptr;
      p.pool_part = nullptr;
    }
  } else {
    tile_of_block(blockIdx.x, nMt, nNt, mt, nt);
  }
  w14p2_tile<NPS, EPI, F16>(p, mt * BM, nt * BN, w, smem3, cb_begin, cb_end, slice);
}

// one thread per (tail row, 4 channels): ordered sum of the K slices, then the usual epilogue (BN scale/shift,
// activation, rowmap compaction, fp32 and/or split-blocked store).  Padding channels (n >= N) are written as zeros.
__global__ void bf16x3_tail_reduce_kernel(GemmArgs p, int mt0, int S) {
  const int quads = p.Npad >> 2;
  const int64_t rows = (int64_t)p.tail_mt * BM;
  const int64_t total = rows * quads;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / quads;
    const int n = (int)(i - r * quads) * 4;
    const int64_t m = (int64_t)mt0 * BM + r;
    if (m >= p.M) continue;
    bool zero;
    const int orow = out_row(p, (int)m, zero);
    if (orow < 0) continue;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s) acc += *reinterpret_cast<const f32x4*>(p.partial + ((int64_t)s * rows + r) * p.Npad + n);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (n + e < p.N && !zero) v[e] = apply_act(fmaf(acc[e], p.scale[n + e], p.shift[n + e]), p.act, p.alpha ? p.alpha[n + e] : 0.f);
    if (p.Y && n < p.N) *reinterpret_cast<f32x4*>(p.Y + (int64_t)orow * p.ldy + n) = v;     // N % 4 == 0 (wide epilogue)
    if (p.Ysb && n < p.ldsb) {
      uint32_t h01, l01, h23, l23;
      v *= p.sb_mul;
      split2(v[0], v[1], h01, l01, p.f16);
      split2(v[2], v[3], h23, l23, p.f16);
      if (p.f16) ovf_report(p.ovf, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
      char* blk = reinterpret_cast<char*>(p.Ysb) + (int64_t)orow * p.ldsb * 4 + (n >> 5) * 128 + (n & 31) * 2;
      *reinterpret_cast<uint2*>(blk) = make_uint2(h01, h23);
      *reinterpret_cast<uint2*>(blk + 64) = make_uint2(l01, l23);
    }
  }
}

#undef XV_GLD
#undef XV_WAIT4

// debug (tools/gemm_trace.py): phase stamps of the launch that XVEC_TRACE_K (and XVEC_TRACE_N) select, 8 per workgroup
// (0-3: kernel phases, 4-7: inside the epilogue)
#ifdef XV_GEMM_TRACE
namespace {
long long* g_trace = nullptr;      // device buffer, kTraceWgs workgroups x 8 stamps
int g_trace_wgs = 0;
constexpr int kTraceWgs = 16384;

void trace_arm(GemmArgs& a, hipStream_t s) {
  static int trace_k = -1, trace_n = 0;
  if (trace_k < 0) {
    const char* e = getenv("XVEC_TRACE_K");
    trace_k = e ? atoi(e) : 0;
    const char* e2 = getenv("XVEC_TRACE_N");
    trace_n = e2 ? atoi(e2) : 0;
  }
  if (trace_k <= 0 || a.K != trace_k || (trace_n != 0 && a.N != trace_n)) return;
  if (!g_trace && hipMalloc(&g_trace, sizeof(long long) * 8 * kTraceWgs) != hipSuccess) g_trace = nullptr;
  const int wgs = ((a.M + BM - 1) / BM) * (a.Npad / BN);
  if (g_trace && wgs <= kTraceWgs) {
    a.trace = g_trace;
    g_trace_wgs = wgs;
    (void)hipMemsetAsync(g_trace, 0, sizeof(long long) * 8 * kTraceWgs, s);
  }
}
void trace_grid(const GemmArgs& a, unsigned wgs) {      // the whole tiles of a launch whose tail tiles go K-split
  if (a.trace) g_trace_wgs = wgs <= (unsigned)kTraceWgs ? (int)wgs : 0;
}
}  // namespace

// not part of the public ABI: copy the phase stamps of the last traced GEMM launch
extern "C" int xvdbg_gemm_trace(long long* out, int max_wgs) {
  if (!g_trace || g_trace_wgs <= 0) return 0;
  const int n = g_trace_wgs < max_wgs ? g_trace_wgs : max_wgs;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpy(out, g_trace, sizeof(long long) * 8 * n, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return n;
}
#else
namespace {
inline void trace_arm(GemmArgs&, hipStream_t) {}
inline void trace_grid(const GemmArgs&, unsigned) {}
}  // namespace
#endif

int64_t gemm_bf16x3_tail_plan(int M, int Kpad, int Npad, int w, int* tail_mt, int* splits, int cb_quant) {
  *tail_mt = 0;
  *splits = 1;
  if (w < 1 || w > 9 || (Kpad >> 5) % w != 0) return 0;          // (switch: xv_set_option "tail_split")
  const int slots = 256 * 3;             // CUs x resident workgroups of the default kernel
  const int nMt = (M + BM - 1) / BM, nNt = Npad / BN, tiles = nMt * nNt, ncb = (Kpad >> 5) / w;
  const int r = tiles % slots;
  if (tiles <= slots || r == 0 || r > slots / 4) return 0;        // only a nearly empty last round is worth splitting
  const int mt = (r + nNt - 1) / nNt;
  int S = 0;
  for (int c = 8; c >= 2; c >>= 1)
    if (ncb % c == 0 && ncb / c >= 2 && (ncb / c) % cb_quant == 0 && mt * nNt * c <= 256) { S = c; break; }   // about one slice workgroup per CU
  if (S == 0) return 0;
  *tail_mt = mt;
  *splits = S;
  return (int64_t)S * mt * BM * Npad * (int64_t)sizeof(float);
}

namespace {
// The instantiation of a kernel form for the split format f16 (bf16 or fp16 hi/lo).  EPI == 3, the producer of the two-unit
// block format, exists in fp16 only: its routes below check a.f16.
template <int NPS, int EPI>
auto w14p2_kernel(bool f16) {
  if constexpr (EPI == 3) return gemm_bf16x3_w14p2_kernel<NPS, 3, true>;
  else return f16 ? gemm_bf16x3_w14p2_kernel<NPS, EPI, true> : gemm_bf16x3_w14p2_kernel<NPS, EPI, false>;
}
template <int EPI, bool GATHER = false>
auto w1p3_kernel(bool f16) {
  if constexpr (EPI == 3) return gemm_bf16x3_w1p3_kernel<3, true, GATHER>;
  else return f16 ? gemm_bf16x3_w1p3_kernel<EPI, true, GATHER> : gemm_bf16x3_w1p3_kernel<EPI, false, GATHER>;
}
}  // namespace

hipError_t launch_gemm_bf16x3(const GemmArgs& a_in, hipStream_t s) {
  if (a_in.M <= 0) return hipSuccess;
  GemmArgs a = a_in;
  trace_arm(a, s);
  static std::mutex init_mu;    // the attributes are per device; any thread may make the first launch on one
  static bool attr_set[64] = {};
  const size_t smemw32 = (size_t)2 * DA_BYTES;      // two slabs; the 4 x 8 KB epilogue scratch overlays them
  const size_t smemw1p3 = (size_t)3 * DA_BYTES;     // one-tap form: three slabs (52 KB, three workgroups per CU)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  {
    std::lock_guard<std::mutex> init_lock(init_mu);
    if (!attr_set[dev & 63]) {
      // every instantiation that a route below can launch (this list is their first use: it fixes their order in the code object)
      const void* kernels[] = {
          reinterpret_cast<const void*>(gemm_bf16x3_w14p2_kernel<1, 0, false>), reinterpret_cast<const void*>(gemm_bf16x3_w14p2_kernel<4, 0, false>),
          reinterpret_cast<const void*>(gemm_bf16x3_w14p2_kernel<4, 1, false>), reinterpret_cast<const void*>(gemm_bf16x3_w14p2_kernel<4, 2, false>),
          reinterpret_cast<const void*>(gemm_bf16x3_w14p2_kernel<1, 0, true>), reinterpret_cast<const void*>(gemm_bf16x3_w14p2_kernel<4, 0, true>),
          reinterpret_cast<const void*>(gemm_bf16x3_w14p2_kernel<4, 1, true>), reinterpret_cast<const void*>(gemm_bf16x3_w14p2_kernel<4, 2, true>),
          reinterpret_cast<const void*>(gemm_bf16x3_w14p2_kernel<1, 3, true>), reinterpret_cast<const void*>(gemm_bf16x3_w14p2_kernel<4, 3, true>)};
      hipError_t r = hipSuccess;
      for (const void* k : kernels) {
        r = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smemw32);
        if (r != hipSuccess) return r;
      }
      const void* kernels3[] = {
          reinterpret_cast<const void*>(gemm_bf16x3_w1p3_kernel<0, false>), reinterpret_cast<const void*>(gemm_bf16x3_w1p3_kernel<0, true>),
          reinterpret_cast<const void*>(gemm_bf16x3_w1p3_kernel<1, false>), reinterpret_cast<const void*>(gemm_bf16x3_w1p3_kernel<1, true>),
          reinterpret_cast<const void*>(gemm_bf16x3_w1p3_kernel<2, false>), reinterpret_cast<const void*>(gemm_bf16x3_w1p3_kernel<2, true>),
          reinterpret_cast<const void*>(gemm_bf16x3_w1p3_kernel<0, false, true>), reinterpret_cast<const void*>(gemm_bf16x3_w1p3_kernel<0, true, true>),
          reinterpret_cast<const void*>(gemm_bf16x3_w1p3_kernel<3, true>), reinterpret_cast<const void*>(gemm_bf16x3_w1p3_kernel<3, true, true>)};
      for (const void* k : kernels3) {
        r = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smemw1p3);
        if (r != hipSuccess) return r;
      }
      attr_set[dev & 63] = true;
    }
  }
  const int w = a.K / a.cin > 0 && a.ldsbx == a.cin ? a.K / a.cin : 1;   // taps (dense: 1)
  const bool taps_ok = w <= 9 && (a.Kpad >> 5) % w == 0;   // slab halo: 128 + w - 1 <= DA_ROWS (136)
  const int nNt = a.Npad / BN, nMt = (a.M + BM - 1) / BM;
  if (!taps_ok) return hipErrorInvalidValue;   // the plan only routes layers of <= 9 taps and whole 32-channel blocks here
  // 1 x 4 waves, weights in registers two steps ahead.  Tail handling is decided at plan time (the plan owns the
  // partial workspace): the last tail_mt M tiles go K-split
  const dim3 block(256);
  if (a.att_part || a.pool_w) {                 // attention epilogue: dense layers without row compaction only
    if (w != 1 || a.rowmap || a.a_pitch || a.R || (a.N & 3) || (a.pool_w && !a.pool_part)) return hipErrorInvalidValue;
    const dim3 grid(nMt * nNt);
    if (!a.slab3) {
      if (a.att_part) hipLaunchKernelGGL((w14p2_kernel<4, 1>(a.f16)), grid, block, smemw32, s, a, nMt, nNt, w, 0);
      else            hipLaunchKernelGGL((w14p2_kernel<4, 2>(a.f16)), grid, block, smemw32, s, a, nMt, nNt, w, 0);
    } else {
      if (a.att_part) hipLaunchKernelGGL((w1p3_kernel<1>(a.f16)), grid, block, smemw1p3, s, a, nMt, nNt);
      else            hipLaunchKernelGGL((w1p3_kernel<2>(a.f16)), grid, block, smemw1p3, s, a, nMt, nNt);
    }
    return hipGetLastError();
  }
  const bool tail = a.tail_mt > 0 && a.ksplit > 1 && a.partial && !a.a_pitch && !a.pool_part && !a.R && !a.raw &&
                    a.tail_mt < nMt && (a.N & 3) == 0;
  const int nMain = tail ? nMt - a.tail_mt : nMt;
  const dim3 grid(nMain * nNt);
  trace_grid(a, grid.x);
  if (a.arow) {                                 // gathered grid rows (ResNet convolutions without border rows)
    if (w != 1 || tail || !a.a_pitch || a.pool_part) return hipErrorInvalidValue;
    // ysb_f6: the reader is a two-unit ResNet convolution: its block format, nothing else
    if (a.ysb_f6 && (!a.f16 || !a.Ysb || a.Y || a.R)) return hipErrorInvalidValue;
    if (a.ysb_f6) hipLaunchKernelGGL((w1p3_kernel<3, true>(a.f16)), grid, block, smemw1p3, s, a, nMain, nNt);
    else          hipLaunchKernelGGL((w1p3_kernel<0, true>(a.f16)), grid, block, smemw1p3, s, a, nMain, nNt);
    return hipGetLastError();
  }
  // ysb_f6 (XV_PREC_F16F6): this layer's only reader is a two-unit layer -> its block format
  if (a.ysb_f6 && (!a.f16 || (w > 1 && w < 5) || !a.Ysb || a.Y || a.R || a.pool_part)) return hipErrorInvalidValue;
  if (w == 1 && !tail && a.slab3) {             // one tap: three slab buffers, slabs two steps ahead
    if (a.ysb_f6) hipLaunchKernelGGL((w1p3_kernel<3>(a.f16)), grid, block, smemw1p3, s, a, nMain, nNt);
    else          hipLaunchKernelGGL((w1p3_kernel<0>(a.f16)), grid, block, smemw1p3, s, a, nMain, nNt);
    return hipGetLastError();
  }
  // whole tiles, then (tail form) the K-split slices of the tail tiles in the same launch: raw sums that a reduce finishes
  const int S = tail ? a.ksplit : 0;
  const dim3 grid2(nMain * nNt + (tail ? a.tail_mt * nNt * a.ksplit : 0));
  if (a.ysb_f6) {
    if (w >= 5) hipLaunchKernelGGL((w14p2_kernel<1, 3>(a.f16)), grid2, block, smemw32, s, a, nMain, nNt, w, S);
    else        hipLaunchKernelGGL((w14p2_kernel<4, 3>(a.f16)), grid2, block, smemw32, s, a, nMain, nNt, w, S);
  } else {
    if (w >= 5) hipLaunchKernelGGL((w14p2_kernel<1, 0>(a.f16)), grid2, block, smemw32, s, a, nMain, nNt, w, S);
    else        hipLaunchKernelGGL((w14p2_kernel<4, 0>(a.f16)), grid2, block, smemw32, s, a, nMain, nNt, w, S);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess || !tail) return e;
  if (a.ysb_f6) return launch_f6v2_tail_reduce(a, nMain, s);      // the two-unit kernel's reduce writes its block format
  const int64_t total = (int64_t)a.tail_mt * BM * (a.Npad >> 2);
  hipLaunchKernelGGL(bf16x3_tail_reduce_kernel, dim3((unsigned)((total + 255) / 256)), block, 0, s, a, nMain, a.ksplit);
  return hipGetLastError();
}

}  // namespace xv
