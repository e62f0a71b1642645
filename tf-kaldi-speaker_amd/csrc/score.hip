// Cosine and PLDA scoring of x-vectors on the GPU: row preparation, score matrices, trial lists, score histograms.
//
// The reference scores in two places, both on the host:
//   egs/voxceleb/v1/run.sh:362-365   ivector-compute-dot-products over length-normalised x-vectors (plain cosine)
//   egs/voxceleb/v1/run.sh:404-408   ivector-subtract-global-mean | transform-vec | ivector-normalize-length in front of it
//   misc/utils.py:307-346            compute_cos_pairwise_eer: embeddings / sqrt(sum x^2 + 1e-12), the full score matrix
//                                    in numpy and a Python double loop over i < j (hence its down-sampling to 1000 rows)
// Kaldi is not part of the reference tree; the Kaldi steps restate the published algorithms (**parity unpinned**, as
// csrc/post.hip), checked against tests/helpers/ref_score.py.
//
// All arithmetic is fp32 with exact products and fp32 accumulation, so one error bound ((d + 8) * 2^-24 per score of
// unit rows) holds for every entry point.
//
// PLDA scoring with a trained Kaldi `Plda` (`ivector-plda-scoring`, the last line of every recipe: egs/voxceleb/v1/run.sh:410-426)
// runs on the same kernels: the log likelihood ratio of plda.cc expands to  s(i, j) = sum_d A_id t_jd + sum_d W_id t_jd^2 + rho_i
// (tf-kaldi-speaker_amd/plda.py has the algebra), i.e. a product of packed rows plus a row term and a column term added in the
// epilogue.  plda_rows_kernel normalises the transformed rows and packs the operands; rho / tau are accumulated in double and
// rounded once.  Training (ivector-compute-lda / -plda) is csrc/backend.hip; ivector-adapt-plda stays with Kaldi.  **Parity unpinned** as well.
//
//  * row_prepare_kernel: one wave per row; y = x - mean, then y / sqrt(sum y^2 + eps).  The sum of squares is taken of
//    the row scaled by the power of two of its largest element (exact), so rows of any magnitude neither overflow nor flush.
//  * score_tile_kernel: C = A * B^T over prepared rows, the exact-fp32 tile product of csrc/nt_gemm.h at 128 x 128 per
//    workgroup, K = d taken whole.  A workgroup walks tiles with a stride of the grid, in the order of ntg::nt_tile.
//    Epilogues (compile time):
//      EPI_MATRIX       fp32 [n, m] with a leading dimension
//      EPI_AFFINE       the same with a vector subtracted from the A rows at load and column d of B added as an offset
//                       (ivector-subtract-global-mean + transform-vec of the prepare step)
//      EPI_HIST_LDS     same-label / different-label histograms of the scores, uint32 counts in LDS (ds_add_u32) for the
//                       whole walk of the workgroup, flushed once with 64-bit vector atomics (2 * nbins * 4 bytes <= 64 KB)
//      EPI_HIST_GLOBAL  the same with one 64-bit vector atomic per score (bin counts that do not fit in LDS)
//      EPI_PLDA         EPI_MATRIX with row_bias[i] + col_bias[j] added before the store (the biases of the tile sit in LDS)
//      EPI_PLDA_HIST_LDS / EPI_PLDA_HIST_GLOBAL   the two histogram epilogues over the biased score and a caller-given range
//                       [lo, hi): bin = clamp(floor((s - lo) * nbins / (hi - lo)), 0, nbins - 1), evaluated in double so that the
//                       bin edges are exact
//    Integer adds commute, so the counts are exact and independent of the order of arrival.
//  * score_pairs_kernel: trial lists.  16 lanes per trial (four trials per wave), 16-byte row loads, four fmaf chains per
//    lane combined in a fixed order and a DPP butterfly over the 16 lanes: repeats are bit-identical.
//    The PLDA form adds row_bias[ia[k]] + col_bias[ib[k]].
//  * plda_rows_kernel: one wave per row, after the affine product of the prepare step (u = transform (x - mean)):
//    y = u * sqrt(D / sum_d u_d^2 inv_d) (Kaldi's TransformIvector; inv = 1 / (psi + 1 / n), or 1 for the simple form), the sum
//    in double so that rows of any fp32 magnitude neither overflow nor flush and a zero row stays zero; then the packed operand
//    y_d p_d (and the second half, W_d on the enrolment side or y_d^2 on the test side, for sets of mixed n) and the bias
//    logdet + sum_d q_d y_d^2.  The per-n vectors inv, p, q, w come from the host in float64, one table per distinct n.
//
// Score normalisation (Z/T/S-norm with adaptive top-K cohorts) and identification (top-K gallery search) want the K largest
// scores of every row, never the [n, m] matrix; include/xvec_hip.h has the definitions.  Both are missing from the reference
// (egs/sre/v1/run.sh:13) and from Kaldi's binaries: **parity unpinned**, checked against tests/helpers/ref_snorm.py and
// ref_topk.py.  They share two things:
//  * the panel walk (walk_panels): score_tile_kernel (EPI_MATRIX, or EPI_PLDA when a bias is given) writes a panel of whole
//    tile rows of scores into the workspace, so every score is the one xv_score_matrix / xv_plda_matrix would write; then a
//    select kernel runs with one workgroup per panel row.  Rows of up to 12288 scores are copied into LDS once (SelRow) and
//    every sweep reads them there; longer rows are swept in global memory (L2).  A fused epilogue that never writes the panel
//    has not been built;
//  * the select (radix_select): exact, on the order-preserving uint32 image of the float (digits of 11, 11 and 10 bits,
//    histograms in LDS with ds_add_u32): the K-th largest eligible score of the row and its multiplicity inside the top K.
//    K = all eligible columns skips it.
// cohort_select_kernel then sums what lies above the K-th score in one sweep and takes the centred squares in one more, both
// in double and in a fixed order.  topk_select_kernel lets the select stop as soon as the candidates fit its sort, compacts
// the hits into LDS in column order and sorts (score, column) keys with a bitonic network.
#include "nt_gemm.h"

namespace xv {

using ntg::gf32x4;

namespace {

constexpr int SBM = 128, SBN = 128;           // the tile of a workgroup
constexpr size_t kOperandBytes = ntg::nt_smem_bytes<SBM, SBN>();
constexpr int kOperandFloats = (int)(kOperandBytes / sizeof(float));
constexpr int kScoreLdsBins = 8192;           // largest bin count whose two uint32 histograms stay in LDS (64 KB) beside the operand tiles
constexpr size_t kLabelBytes = (size_t)(SBM + SBN) * sizeof(int32_t);

constexpr size_t kBiasBytes = (size_t)(SBM + SBN) * sizeof(float);

enum { EPI_MATRIX = 0, EPI_AFFINE = 1, EPI_HIST_LDS = 2, EPI_HIST_GLOBAL = 3, EPI_PLDA = 4, EPI_PLDA_HIST_LDS = 5, EPI_PLDA_HIST_GLOBAL = 6 };

constexpr bool epi_hist(int e) { return e == EPI_HIST_LDS || e == EPI_HIST_GLOBAL || e == EPI_PLDA_HIST_LDS || e == EPI_PLDA_HIST_GLOBAL; }
constexpr bool epi_hist_lds(int e) { return e == EPI_HIST_LDS || e == EPI_PLDA_HIST_LDS; }
constexpr bool epi_plda(int e) { return e == EPI_PLDA || e == EPI_PLDA_HIST_LDS || e == EPI_PLDA_HIST_GLOBAL; }

// ---------------------------------------------------------------------------------------------- prepare
__global__ __launch_bounds__(256) void row_prepare_kernel(const float* __restrict__ x, int64_t ldx, int64_t rows, int dim,
                                                          const float* __restrict__ mean, int normalize, float eps,
                                                          float* __restrict__ y, int64_t ldy) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float* xr = x + r * ldx;
  float* yr = y + r * ldy;
  auto at = [&](int c) { return mean ? xr[c] - mean[c] : xr[c]; };
  if (!normalize) {
    for (int c = lane; c < dim; c += 64) yr[c] = at(c);
    return;
  }
  float mx = 0.f;
  for (int c = lane; c < dim; c += 64) mx = fmaxf(mx, fabsf(at(c)));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if (!(mx > 0.f) || !(mx <= 3.4028234e38f)) {     // zero row: stays zero (eps == 0) or is zero anyway; inf / nan rows: copied
    for (int c = lane; c < dim; c += 64) yr[c] = at(c);
    return;
  }
  const int e = ilogbf(mx);                         // row * 2^-e has its largest element in [1, 2): exact scaling
  float ss = 0.f;
  for (int c = lane; c < dim; c += 64) {
    const float v = ldexpf(at(c), -e);
    ss = fmaf(v, v, ss);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  // x / sqrt(sum x^2 + eps) = (x 2^-e) / sqrt(ss + eps 2^-2e); where eps 2^-2e is out of range the sum of squares is
  // far below one ulp of eps and the row is x / sqrt(eps)
  const float es = ldexpf(ldexpf(eps, -e), -e);
  if (es <= 3.4028234e38f) {
    const float inv = 1.0f / sqrtf(ss + es);
    for (int c = lane; c < dim; c += 64) yr[c] = ldexpf(at(c), -e) * inv;
  } else {
    const float inv = 1.0f / sqrtf(eps);
    for (int c = lane; c < dim; c += 64) yr[c] = at(c) * inv;
  }
}

// ---------------------------------------------------------------------------------------------- tiles
struct ScoreArgs {
  const float* A; int64_t lda; int n;
  const float* B; int64_t ldb; int m;
  int d;
  float* C; int64_t ldc;                 // matrix epilogues
  const float* a_sub;                    // EPI_AFFINE: subtracted from every A row (or null)
  int b_offset;                          // EPI_AFFINE: column d of B is added to the output column
  const int32_t* la; const int32_t* lb;  // histogram epilogues
  int self, nbins;
  unsigned long long* hs; unsigned long long* hd;
  int nMt, nNt;
  const float* row_bias; const float* col_bias;   // PLDA epilogues: rho [n], tau [m] (tau may be null: 0)
  double lo, bin_scale;                           // PLDA histograms: bin = floor((s - lo) * bin_scale)
};

template <int EPI, bool VEC>
__global__ __launch_bounds__(256, 2) void score_tile_kernel(ScoreArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int32_t* lab = reinterpret_cast<int32_t*>(smem + kOperandFloats);       // [SBM + SBN] labels of the tile
  unsigned* hist = reinterpret_cast<unsigned*>(lab + SBM + SBN);          // EPI_HIST_LDS: [2][nbins]
  // PLDA: [SBM + SBN] biases of the tile, behind whatever the epilogue keeps in front of them
  float* bias = EPI == EPI_PLDA ? smem + kOperandFloats
                                : reinterpret_cast<float*>(hist + (EPI == EPI_PLDA_HIST_LDS ? 2 * p.nbins : 0));

  const int tid = threadIdx.x;
  const float half_bins = 0.5f * (float)p.nbins;

  if (epi_hist_lds(EPI)) {
    for (int i = tid; i < 2 * p.nbins; i += 256) hist[i] = 0u;
    __syncthreads();
  }

  const int64_t ntiles = (int64_t)p.nMt * p.nNt;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    int mt, nt;
    ntg::nt_tile(t, p.nMt, p.nNt, mt, nt);
    if (epi_hist(EPI) && p.self && nt < mt) continue;   // strictly below the diagonal (uniform)
    const ntg::NtPos<SBM, SBN> at(mt, nt);
    const int m0 = at.m0, n0 = at.n0;

    if (epi_hist(EPI) && !epi_plda(EPI)) {
      const int row = tid < SBM ? m0 + tid : n0 + tid - SBM;
      const bool ok = tid < SBM ? row < p.n : row < p.m;
      lab[tid] = ok ? (tid < SBM ? p.la[row] : p.lb[row]) : 0;
    }
    if (epi_plda(EPI)) {
      const bool rowside = __builtin_amdgcn_readfirstlane(tid) < SBM;     // waves 0-1: rows, waves 2-3: columns; the bases stay scalar
      const float* src = rowside ? p.row_bias : p.col_bias;
      const int row = rowside ? m0 + tid : n0 + tid - SBM;
      const bool ok = row < (rowside ? p.n : p.m);
      bias[tid] = src && ok ? src[row] : 0.f;
      if (epi_hist(EPI)) lab[tid] = ok ? (rowside ? p.la : p.lb)[row] : 0;
    }

    ntg::gf32x16 acc[2][2];            // acc[ai][bi]: 32 A rows x 32 B rows
    ntg::nt_acc_start(acc, at);
    // its first barrier publishes the labels / biases too
    ntg::nt_mainloop<SBM, SBN, VEC, EPI == EPI_AFFINE>(p.A, p.lda, p.n, p.B, p.ldb, p.m, p.d, m0, n0, acc, smem, p.a_sub);

#pragma unroll
    for (int bi = 0; bi < 2; ++bi) {
      const int jl = at.lcol(bi);
      const int gj = n0 + jl;
      if (gj >= p.m) continue;
      float offs = 0.f;
      int lbj = 0;
      if (EPI == EPI_AFFINE) offs = p.b_offset ? p.B[(int64_t)gj * p.ldb + p.d] : 0.f;
      if (epi_hist(EPI)) lbj = lab[SBM + jl];
      float cb = 0.f;
      if (epi_plda(EPI)) cb = bias[SBM + jl];
#pragma unroll
      for (int ai = 0; ai < 2; ++ai)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int il = at.lrow(ai, e);
          const int gi = m0 + il;
          if (gi >= p.n) continue;
          float s = acc[ai][bi][e];
          if (epi_plda(EPI)) s = (s + bias[il]) + cb;
          if (EPI == EPI_MATRIX || EPI == EPI_AFFINE) {
            p.C[(int64_t)gi * p.ldc + gj] = s + offs;
          } else if (EPI == EPI_PLDA) {
            p.C[(int64_t)gi * p.ldc + gj] = s;
          } else {
            if (p.self && gi >= gj) continue;
            int bin;
            if (epi_plda(EPI)) {      // truncation is floor where it is used; a NaN score lands in bin 0
              const double fb = ((double)s - p.lo) * p.bin_scale;
              bin = fb >= (double)p.nbins ? p.nbins - 1 : (fb >= 1.0 ? (int)fb : 0);
            } else {
              const float fb = fminf(fmaxf(floorf((s + 1.0f) * half_bins), 0.f), (float)(p.nbins - 1));
              bin = (int)fb;
            }
            const bool same = lab[il] == lbj;
            if (epi_hist_lds(EPI))
              atomicAdd(&hist[(same ? 0 : p.nbins) + bin], 1u);
            else
              atomicAdd((same ? p.hs : p.hd) + bin, 1ull);
          }
        }
    }
    if (epi_hist(EPI) || epi_plda(EPI)) __syncthreads();     // the labels / biases are rewritten by the next tile
  }

  if (epi_hist_lds(EPI)) {
    __syncthreads();
    for (int i = tid; i < 2 * p.nbins; i += 256) {
      const unsigned c = hist[i];
      if (c) atomicAdd(i < p.nbins ? p.hs + i : p.hd + (i - p.nbins), (unsigned long long)c);
    }
  }
}

template <int EPI>
hipError_t launch_tiles_v(const ScoreArgs& a, unsigned grid, size_t smem, hipStream_t s) {
  return ntg::nt_vec(a.A, a.lda, a.B, a.ldb) ? ntg::nt_launch<score_tile_kernel<EPI, true>>(smem, grid, a, s)
                                             : ntg::nt_launch<score_tile_kernel<EPI, false>>(smem, grid, a, s);
}

// ---------------------------------------------------------------------------------------------- pairs
template <bool VEC, bool PLDA>
__global__ __launch_bounds__(256) void score_pairs_kernel(const float* __restrict__ a, int64_t lda, int n,
                                                          const float* __restrict__ b, int64_t ldb, int m, int d,
                                                          const int32_t* __restrict__ ia, const int32_t* __restrict__ ib,
                                                          int64_t npairs, float* __restrict__ out,
                                                          const float* __restrict__ row_bias, const float* __restrict__ col_bias) {
  const int sub = threadIdx.x & 15;
  const int64_t k = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool have = k < npairs;
  const int i = have ? ia[k] : 0, j = have ? ib[k] : 0;
  const bool ok = have && i >= 0 && i < n && j >= 0 && j < m;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (ok) {
    const float* x = a + (int64_t)i * lda;
    const float* y = b + (int64_t)j * ldb;
    for (int c = sub * 4; c < d; c += 64) {
      if (VEC && c + 4 <= d) {
        const gf32x4 u = *reinterpret_cast<const gf32x4*>(x + c);
        const gf32x4 v = *reinterpret_cast<const gf32x4*>(y + c);
        s0 = fmaf(u[0], v[0], s0);
        s1 = fmaf(u[1], v[1], s1);
        s2 = fmaf(u[2], v[2], s2);
        s3 = fmaf(u[3], v[3], s3);
      } else {
        if (c < d) s0 = fmaf(x[c], y[c], s0);
        if (c + 1 < d) s1 = fmaf(x[c + 1], y[c + 1], s1);
        if (c + 2 < d) s2 = fmaf(x[c + 2], y[c + 2], s2);
        if (c + 3 < d) s3 = fmaf(x[c + 3], y[c + 3], s3);
      }
    }
  }
  float s = row16_sum((s0 + s1) + (s2 + s3));            // every lane of the wave takes part
  if (PLDA && ok) s = (s + row_bias[i]) + (col_bias ? col_bias[j] : 0.f);
  if (have && sub == 0) out[k] = ok ? s : __builtin_nanf("");  // an index the host let through is marked, never followed
}

// ---------------------------------------------------------------------------------------------- PLDA rows
constexpr int PT_INV = 0, PT_P = 1, PT_Q = 2, PT_W = 3;      // components of a per-n table [4][d] (doubles)

// norm: 0 none, 1 Kaldi's psi-weighted length normalisation (inv table), 2 simple (sqrt(d) / ||u||).
// side: 0 enrolment (second half of the packed row = W), 1 test (second half = y^2).  Any output may be null; rows == u is allowed.
__global__ __launch_bounds__(256) void plda_rows_kernel(const float* u, int64_t ldu, int64_t nrows, int d, int norm,
                                                        int side, int pack_second, const double* __restrict__ tables,
                                                        const double* __restrict__ logdet, const int32_t* __restrict__ table_index,
                                                        int num_tables, float* rows, int64_t ldr, float* __restrict__ packed,
                                                        int64_t ldp, float* __restrict__ bias) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= nrows) return;
  int k = table_index ? table_index[r] : 0;
  if (k < 0 || k >= num_tables) k = 0;              // the host checks; never followed out of the tables
  const double* tab = tables + (int64_t)k * 4 * d;
  const float* ur = u + r * ldu;
  double scale = 1.0;
  if (norm) {
    double ss = 0.0;
    for (int c = lane; c < d; c += 64) {
      const double v = (double)ur[c];
      ss = fma(v * v, norm == 1 ? tab[PT_INV * d + c] : 1.0, ss);
    }
    ss = wave_sum_f64(ss);
    // a zero row stays zero; a row with inf / nan is passed through
    scale = ss > 0.0 ? (ss <= 1.7976931348623157e308 ? sqrt((double)d / ss) : 1.0) : (ss == 0.0 ? 0.0 : 1.0);
  }
  double acc = 0.0;
  for (int c = lane; c < d; c += 64) {
    const float y = (float)((double)ur[c] * scale);
    const double y2 = (double)y * (double)y;
    acc = fma(tab[PT_Q * d + c], y2, acc);
    if (rows) rows[r * ldr + c] = y;
    if (packed) {
      packed[r * ldp + c] = (float)((double)y * tab[PT_P * d + c]);
      if (pack_second) packed[r * ldp + d + c] = side == 0 ? (float)tab[PT_W * d + c] : (float)y2;
    }
  }
  acc = wave_sum_f64(acc);
  if (bias && lane == 0) bias[r] = (float)((logdet ? logdet[k] : 0.0) + acc);
}

// ---------------------------------------------------------------------------------------------- row select
constexpr int kSelBins = 2048;                // digit histogram of the radix select: digits of 11, 11 and 10 bits
constexpr int kSelStageMax = 12288;           // rows of up to this many scores are kept in LDS for all sweeps (48 KB)
constexpr int kTopkMax = 1024;                // keys of the top-K sort: 8 KB, the bytes of the digit histogram they take over

// dynamic LDS of the two select kernels: this fixed region, then the staged row [m] when STAGE
struct SelLds {
  unsigned hist[kSelBins];                    // digit histogram; top-K: the 64-bit sort keys [kTopkMax] once the select is done
  double dslot[8];                            // two block_sum slots of the statistics
  unsigned uslot[8];                          // 0-3 wave sums; the select: 4 digit found, 5 rank left in it, 6 scores down to it
  __device__ float* stage() { return reinterpret_cast<float*>(this + 1); }
};
constexpr size_t kSelFixedBytes = sizeof(SelLds);
static_assert(kTopkMax * sizeof(unsigned long long) <= sizeof(SelLds::hist), "the keys reuse the histogram");

// order-preserving uint32 image of a float: a < b  <=>  key(a) < key(b); -0.0 and +0.0 share the key of +0.0
__device__ __forceinline__ unsigned score_key(float v) {
  unsigned u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float score_unkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// sum over the workgroup (4 waves), the same bits in every thread and in every run: xor butterfly per wave, then the four
// wave sums in a fixed order.  `slot` [4] is LDS of the caller; it is free again when the call returns.
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* slot) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  const T r = (slot[0] + slot[1]) + (slot[2] + slot[3]);
  __syncthreads();
  return r;
}

// One row of a panel of scores [rows, ldp], as the workgroup of a select kernel sees it: the row is copied into LDS once when
// STAGE, and every later sweep reads it there; a column j is eligible unless la[row] == lb[j]; `elig` counts the eligible columns.
template <bool STAGE>
struct SelRow {
  const float* src;
  const float* stage;
  const int32_t* lb;
  int32_t mine;
  bool excl;
  unsigned elig;
  __device__ __forceinline__ SelRow(SelLds* lds, const float* panel, int64_t ldp, int m, const int32_t* la, const int32_t* lb_)
      : src(panel + (int64_t)blockIdx.x * ldp), stage(lds->stage()), lb(lb_), mine(0), excl(la != nullptr), elig((unsigned)m) {
    const int tid = threadIdx.x;
    if (STAGE) {
      float* st = lds->stage();
      for (int j = tid; j < m; j += 256) st[j] = src[j];
      __syncthreads();
    }
    mine = excl ? la[blockIdx.x] : 0;
    if (excl) {
      unsigned c = 0;
      for (int j = tid; j < m; j += 256) c += lb[j] != mine ? 1u : 0u;
      elig = block_sum(c, lds->uslot);
    }
  }
  __device__ __forceinline__ float val(int j) const { return STAGE ? stage[j] : src[j]; }
  __device__ __forceinline__ bool eligible(int j) const { return !excl || lb[j] != mine; }
};

// What the radix select finds: the key T of the K-th largest eligible score and how many copies of it (`ties`) belong to the
// top K.  With an early stop: `ncand` scores go on to the sort, and `whole_digit` says they are all scores with a key >= T,
// more than K of them (T is then the lowest key of the digit: the bits below it are zero).
struct SelCut {
  unsigned T, ties, ncand;
  bool whole_digit;
};

// Exact radix select of the K-th largest eligible score of a row (0 < K < eligible) on score_key, by the whole workgroup:
// three passes over digits of 11, 11 and 10 bits.  A pass counts, in an LDS histogram (ds_add_u32; integer counts commute), the
// digit of every score whose key matches the prefix fixed so far, then walks the digits downwards to the one that holds the
// rank-th largest.  `sweep(tally)` calls tally(j, v) for every column j of the row with its score v, in any order.
// STOP > 0 ends the select after a pass (not the last) when everything from the digit it has just fixed upwards is at most
// STOP scores: there is nothing to refine when all of them fit the caller's sort (the usual case of a small K in a long row:
// one sweep instead of three).  STOP == 0: no early stop, and neither its LDS word nor its compare exist.
template <unsigned STOP, typename Row, typename Sweep>
__device__ __forceinline__ SelCut radix_select(SelLds* lds, const Row& row, unsigned K, Sweep sweep) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned* hist = lds->hist;
  unsigned* uslot = lds->uslot;
  SelCut cut = {0u, 0u, K, false};
  unsigned prefix = 0u, mask = 0u, rank = K;     // the rank-th largest of the scores whose key matches prefix under mask
#pragma unroll 1
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = pass == 0 ? 21 : (pass == 1 ? 10 : 0);
    const unsigned dmask = pass == 2 ? 0x3ffu : 0x7ffu;
    for (int i = tid; i < kSelBins; i += 256) hist[i] = 0u;
    __syncthreads();
    sweep([&](int j, float v) {
      if (!row.eligible(j)) return;
      const unsigned key = score_key(v);
      if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & dmask], 1u);
    });
    __syncthreads();
    // thread t owns digits 2047 - 8 t down to 2040 - 8 t; an inclusive scan over the threads walks the digits downwards
    const int top = kSelBins - 1 - 8 * tid;
    unsigned c[8], mysum = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      c[i] = hist[top - i];
      mysum += c[i];
    }
    unsigned incl = mysum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned y = __shfl_up(incl, o, 64);
      if (lane >= o) incl += y;
    }
    if (lane == 63) uslot[wave] = incl;
    __syncthreads();
    for (int w = 0; w < wave; ++w) incl += uslot[w];
    unsigned above = incl - mysum;               // matching scores in the digits above this thread's
    if (above < rank && rank <= incl) {          // exactly one thread: the counts below rank are monotone
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (above + c[i] >= rank) {
          uslot[4] = (unsigned)(top - i);
          uslot[5] = rank - above;
          if (STOP) uslot[6] = above + c[i];     // matching scores down to and including this digit
          break;
        }
        above += c[i];
      }
    }
    __syncthreads();
    // K - rank scores lie above the prefix group, uslot[6] more from this digit upwards inside it.  Uniform: every operand
    // comes from LDS.
    const unsigned from_here_up = STOP ? (K - rank) + uslot[6] : 0u;
    prefix |= uslot[4] << shift;
    mask |= dmask << shift;
    rank = uslot[5];
    if (STOP && pass < 2 && from_here_up <= STOP) {
      cut.whole_digit = true;
      cut.ncand = from_here_up;
      break;
    }
  }
  cut.T = prefix;
  cut.ties = rank;
  return cut;
}

// ---------------------------------------------------------------------------------------------- cohort statistics
// One workgroup per row of a panel of scores [rows, ldp]: mean and population standard deviation of the K largest eligible
// scores of the row (K = top_k, or all of them for top_k == 0, capped by the number of eligible columns).  radix_select fixes
// the key T of the K-th largest score and how many copies of it belong to the top K; the sums then take every score above T
// and that many copies of T.  Mean and centred sum of squares are accumulated in double, thread-strided and combined in a
// fixed order, and rounded once.
template <bool STAGE>
__global__ __launch_bounds__(256) void cohort_select_kernel(const float* __restrict__ panel, int64_t ldp, int m,
                                                            const int32_t* __restrict__ la, const int32_t* __restrict__ lb,
                                                            int top_k, float* __restrict__ mean, float* __restrict__ stdv,
                                                            int32_t* __restrict__ count) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sel_raw[];
  SelLds* lds = reinterpret_cast<SelLds*>(sel_raw);
  const int tid = threadIdx.x;
  const int64_t r = blockIdx.x;
  const SelRow<STAGE> row(lds, panel, ldp, m, la, lb);
  const unsigned elig = row.elig;
  const unsigned K = top_k > 0 && (unsigned)top_k < elig ? (unsigned)top_k : elig;      // top_k == 0: all of them
  if (K == 0) {                                  // uniform: nothing to take the statistics of
    if (tid == 0) {
      mean[r] = __builtin_nanf("");
      stdv[r] = __builtin_nanf("");
      if (count) count[r] = 0;
    }
    return;
  }

  const bool all = K == elig;
  SelCut cut = {};
  if (!all) {
    cut = radix_select<0u>(lds, row, K, [&](auto tally) {
      for (int j = tid; j < m; j += 256) tally(j, row.val(j));
    });
  }
  const unsigned T = cut.T, ties = cut.ties;
  const double tval = (double)score_unkey(T);

  double acc = 0.0;
  for (int j = tid; j < m; j += 256) {
    if (!row.eligible(j)) continue;
    const float v = row.val(j);
    if (all || score_key(v) > T) acc += (double)v;
  }
  double total = block_sum(acc, lds->dslot);
  if (!all) total += (double)ties * tval;
  const double mu = total / (double)K;

  acc = 0.0;
  for (int j = tid; j < m; j += 256) {
    if (!row.eligible(j)) continue;
    const float v = row.val(j);
    if (all || score_key(v) > T) {
      const double dv = (double)v - mu;
      acc = fma(dv, dv, acc);
    }
  }
  double ss = block_sum(acc, lds->dslot + 4);
  if (!all) ss += (double)ties * ((tval - mu) * (tval - mu));
  if (tid == 0) {
    mean[r] = (float)mu;
    stdv[r] = (float)sqrt(ss / (double)K);
    if (count) count[r] = (int32_t)K;
  }
}

// ---------------------------------------------------------------------------------------------- top-K search
constexpr int kTopkChunk = 128;               // keys one wave sorts in registers: two per lane

// compare-exchange steps j = 64 .. 1 of the bitonic merges k = k_lo .. k_hi (powers of two, k_lo <= k_hi) on the 128 keys a
// wave holds in registers: lane l has element i0 = base + l in x0 and i0 + 64 in x1.  Descending: in a block with
// (i & k) == 0 the larger key moves to the lower index.  j = 64 pairs a lane's own two keys; below it the partner sits in
// lane l ^ j (a 64-bit shuffle: no LDS bank is touched).  k = 128 starts at j = 64, a smaller k at j = k / 2.
__device__ __forceinline__ void topk_sort_local(unsigned long long& x0, unsigned long long& x1, int i0, int lane, int k_lo,
                                                int k_hi) {
  for (int k = k_lo; k <= k_hi; k <<= 1) {
    const bool desc0 = (i0 & k) == 0, desc1 = ((i0 + 64) & k) == 0;      // equal unless k == 64
    if (k > 64) {
      const unsigned long long hi = x0 > x1 ? x0 : x1, lo = x0 > x1 ? x1 : x0;
      x0 = desc0 ? hi : lo;
      x1 = desc0 ? lo : hi;
    }
    for (int j = k > 64 ? 32 : k >> 1; j > 0; j >>= 1) {
      const unsigned long long y0 = __shfl_xor(x0, j, 64), y1 = __shfl_xor(x1, j, 64);
      const bool lower = (lane & j) == 0;
      x0 = (lower == desc0) ? (x0 > y0 ? x0 : y0) : (x0 > y0 ? y0 : x0);
      x1 = (lower == desc1) ? (x1 > y1 ? x1 : y1) : (x1 > y1 ? y1 : x1);
    }
  }
}

// One workgroup per row of a panel of scores [rows, ldp]: the K = min(top_k, eligible) largest eligible scores of the row and
// their columns, by score descending and by column ascending among equal scores (a column j is eligible unless
// la[row] == lb[j]); positions K .. top_k - 1 get -inf / -1.  Four steps:
//  1. radix_select fixes the key T of the K-th largest score and how many copies of it (`ties`) belong to the top K.  It stops
//     early when everything from the digit it has just fixed upwards is at most 1024 scores: those are then all candidates
//     (`whole_digit`, more than K of them) and the sort picks the K best, ties included;
//  2. an ordered compaction: wave w owns the w-th quarter of the columns and walks it in column order, so a ballot and a count
//     of the lower lanes (v_mbcnt) number the hits of a walk.  A first walk counts per wave, a prefix over the four counts
//     gives every wave its base, a second walk writes the 64-bit key (score_key << 32 | ~column) of every score above T and
//     of the first `ties` scores equal to T in column order.  No atomic counter: a slot depends on the data alone;
//  3. a bitonic sort of the candidates, padded with zeros (below every real key: ~column has its top bit set) to a power of two
//     P >= 128.  Merge steps with a distance of 128 or more go through LDS, a thread reading and writing keys[i] and
//     keys[i + j] with consecutive lanes on consecutive 8-byte keys: the 32 lanes of a ds_read_b64 group cover one 256-byte
//     bank row and the 16 lanes of a ds_write_b64 group 128 bytes, both conflict-free.  Steps with a smaller distance would
//     fold two lanes of a group onto one bank, so they run in registers (topk_sort_local), 128 keys per wave;
//  4. thread p writes output position p: the column from the key, the score read back from the row (the bits the panel holds,
//     -0.0 included).
// The keys take over the bytes of the digit histogram, which is dead after step 1.  A row too long for LDS is swept in global
// memory with 16-byte loads, four in flight per thread, when the workspace is 16-byte aligned (`vec`; panel rows are padded
// to 4 floats): one 4-byte load per thread and sweep step leaves the walk bound by memory latency.
template <bool STAGE>
__global__ __launch_bounds__(256) void topk_select_kernel(const float* __restrict__ panel, int64_t ldp, int m,
                                                          const int32_t* __restrict__ la, const int32_t* __restrict__ lb,
                                                          int top_k, float* __restrict__ scores, int32_t* __restrict__ index,
                                                          int64_t ldo, int32_t* __restrict__ count, int vec) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sel_raw[];
  SelLds* lds = reinterpret_cast<SelLds*>(sel_raw);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(lds->hist);     // [kTopkMax], steps 2-4
  unsigned* uslot = lds->uslot;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r = blockIdx.x;
  const SelRow<STAGE> row(lds, panel, ldp, m, la, lb);
  const float* src = row.src;
  const unsigned elig = row.elig;
  const unsigned K = (unsigned)top_k < elig ? (unsigned)top_k : elig;              // top_k >= 1
  float* out_s = scores + r * ldo;
  int32_t* out_i = index + r * ldo;
  if (tid == 0 && count) count[r] = (int32_t)K;
  if (K == 0) {                                  // uniform: a fully padded row
    for (int p = tid; p < top_k; p += 256) {
      out_s[p] = -__builtin_inff();
      out_i[p] = -1;
    }
    return;
  }

  const bool all = K == elig;
  SelCut cut = {0u, 0u, K, false};               // all: every eligible score goes into the sort
  if (!all) {                                    // step 1
    cut = radix_select<(unsigned)kTopkMax>(lds, row, K, [&](auto tally) {
      if (!STAGE && vec) {                       // a long row in global memory: four 16-byte loads in flight per thread
        const gf32x4* src4 = reinterpret_cast<const gf32x4*>(src);
        const int m4 = m >> 2;
        for (int q0 = 0; q0 < m4; q0 += 1024) {
          gf32x4 v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int q = q0 + u * 256 + tid;
            v[u] = q < m4 ? src4[q] : gf32x4{0.f, 0.f, 0.f, 0.f};
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int q = q0 + u * 256 + tid;
            if (q < m4) {
#pragma unroll
              for (int e = 0; e < 4; ++e) tally(4 * q + e, v[u][e]);
            }
          }
        }
        for (int j = 4 * m4 + tid; j < m; j += 256) tally(j, src[j]);
      } else {
        for (int j = tid; j < m; j += 256) tally(j, row.val(j));
      }
    });
    __syncthreads();                             // uslot and the histogram are rewritten below
  }
  const unsigned T = cut.T, ties = cut.ties, ncand = cut.ncand;
  const bool whole_digit = cut.whole_digit;

  // step 2: wave w owns columns [w * seg, (w + 1) * seg), seg a multiple of 1024.  A walk takes 64 columns at a time, one per
  // lane, or, for a long row in global memory, 1024 at a time as four 16-byte loads per lane (lane l holds columns
  // 4 l .. 4 l + 3 of each 256): the hits below a column are those of the lower lanes in all four components plus the lane's
  // own lower components.
  const int64_t seg = (((int64_t)m + 3) / 4 + 1023) / 1024 * 1024;
  const int c_lo = (int)(wave * seg < m ? wave * seg : m), c_hi = (int)((wave + 1) * seg < m ? (wave + 1) * seg : m);
  auto classify = [&](int j, float v, bool& g, bool& e) {
    g = e = false;
    if (j < c_hi && row.eligible(j)) {
      const unsigned key = score_key(v);
      g = all || (whole_digit ? key >= T : key > T);
      e = !all && !whole_digit && key == T;
    }
  };
  auto below = [&](unsigned long long b) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
  };
  unsigned gbase = 0u, ebase = 0u, gtotal = 0u;
  // walk(false) counts into gbase / ebase; walk(true) writes the keys from the bases it is given
  auto walk = [&](bool write) {
    auto place = [&](int j, float v, bool g, bool e, unsigned rank_g, unsigned rank_e) {
      if (!(g || e)) return;
      const unsigned slot = g ? gbase + rank_g : gtotal + ebase + rank_e;
      // gtotal + ties == ncand by the select; the bounds keep a slot inside the keys whatever the data
      if ((g || ebase + rank_e < ties) && slot < ncand)
        keys[slot] = ((unsigned long long)score_key(v) << 32) | (unsigned)~(unsigned)j;
    };
    if (!STAGE && vec) {
      const int a_hi = c_hi & ~3;                // c_lo is a multiple of 4; the last m % 4 columns are walked one by one
      for (int j0 = c_lo; j0 < a_hi; j0 += 1024) {
        gf32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int j = j0 + u * 256 + 4 * lane;
          v[u] = j < a_hi ? *reinterpret_cast<const gf32x4*>(src + j) : gf32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int j = j0 + u * 256 + 4 * lane;
          bool g[4], e[4];
          unsigned rank_g = 0u, rank_e = 0u, ng = 0u, ne = 0u;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            classify(j < a_hi ? j + c : c_hi, v[u][c], g[c], e[c]);
            const unsigned long long bg = __ballot(g[c]), be = __ballot(e[c]);
            rank_g += below(bg);
            rank_e += below(be);
            ng += (unsigned)__popcll(bg);
            ne += (unsigned)__popcll(be);
          }
          if (write) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              place(j + c, v[u][c], g[c], e[c], rank_g, rank_e);
              rank_g += g[c] ? 1u : 0u;
              rank_e += e[c] ? 1u : 0u;
            }
          }
          gbase += ng;
          ebase += ne;
        }
      }
    }
    for (int j0 = (!STAGE && vec) ? (c_lo > (c_hi & ~3) ? c_lo : (c_hi & ~3)) : c_lo; j0 < c_hi; j0 += 64) {
      bool g, e;
      const int j = j0 + lane;
      const float v = j < c_hi ? row.val(j) : 0.f;
      classify(j, v, g, e);
      const unsigned long long bg = __ballot(g), be = __ballot(e);
      if (write) place(j, v, g, e, below(bg), below(be));
      gbase += (unsigned)__popcll(bg);
      ebase += (unsigned)__popcll(be);
    }
  };
  walk(false);
  if (lane == 0) {
    uslot[wave] = gbase;
    uslot[4 + wave] = ebase;
  }
  __syncthreads();
  gbase = ebase = 0u;
  for (int w = 0; w < 4; ++w) {
    if (w < wave) {
      gbase += uslot[w];
      ebase += uslot[4 + w];
    }
    gtotal += uslot[w];
  }
  walk(true);
  int P = kTopkChunk;
  while (P < (int)ncand) P <<= 1;
  for (int i = (int)ncand + tid; i < P; i += 256) keys[i] = 0ull;
  __syncthreads();

  // step 3
  auto local_phase = [&](int k_lo, int k_hi) {
    for (int base = wave * kTopkChunk; base < P; base += 4 * kTopkChunk) {
      unsigned long long x0 = keys[base + lane], x1 = keys[base + 64 + lane];
      topk_sort_local(x0, x1, base + lane, lane, k_lo, k_hi);
      keys[base + lane] = x0;
      keys[base + 64 + lane] = x1;
    }
    __syncthreads();
  };
  local_phase(2, kTopkChunk);
  for (int k = 2 * kTopkChunk; k <= P; k <<= 1) {
    for (int j = k >> 1; j >= kTopkChunk; j >>= 1) {
      for (int t = tid; t < P / 2; t += 256) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const unsigned long long x = keys[i], y = keys[i + j];
        if ((x < y) == ((i & k) == 0)) {
          keys[i] = y;
          keys[i + j] = x;
        }
      }
      __syncthreads();
    }
    local_phase(k, k);
  }

  // step 4
  for (int p = tid; p < top_k; p += 256) {
    float s = -__builtin_inff();
    int32_t c = -1;
    if (p < (int)K) {
      c = (int32_t)~(unsigned)keys[p];
      s = row.val(c);
    }
    out_s[p] = s;
    out_i[p] = c;
  }
}

}  // namespace

hipError_t compute_units(int* cus) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  return hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev);
}

hipError_t launch_score_prepare_rows(const float* x, int64_t ldx, int64_t rows, int dim, const float* mean, int normalize,
                                     float eps, float* y, int64_t ldy, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(row_prepare_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, ldx, rows, dim, mean, normalize,
                     eps, y, ldy);
  return hipGetLastError();
}

// operands of a tile launch: rows a [n, d] against rows b [m, d]; everything an epilogue wants is left zero
static ScoreArgs score_args(const float* a, int64_t lda, int n, const float* b, int64_t ldb, int m, int d) {
  ScoreArgs p = {};
  p.A = a; p.lda = lda; p.n = n; p.B = b; p.ldb = ldb; p.m = m; p.d = d;
  p.nMt = (n + SBM - 1) / SBM;
  p.nNt = (m + SBN - 1) / SBN;
  return p;
}

// the matrix epilogues: EPI_AFFINE when the operands ask for it, EPI_PLDA (`plda`: the biases of p, either may be null) or
// EPI_MATRIX; up to 16 workgroups per CU walk the tiles
static hipError_t launch_matrix_tiles(const ScoreArgs& p, bool plda, hipStream_t s) {
  int cus = 0;
  const hipError_t e = compute_units(&cus);
  if (e != hipSuccess) return e;
  const int64_t ntiles = (int64_t)p.nMt * p.nNt;
  const unsigned grid = (unsigned)(ntiles < (int64_t)cus * 16 ? ntiles : (int64_t)cus * 16);
  if (p.a_sub || p.b_offset) return launch_tiles_v<EPI_AFFINE>(p, grid, kOperandBytes, s);
  if (plda) return launch_tiles_v<EPI_PLDA>(p, grid, kOperandBytes + kBiasBytes, s);
  return launch_tiles_v<EPI_MATRIX>(p, grid, kOperandBytes, s);
}

// the histogram epilogues, over the cosine (PLDA false) or the biased score: counts in LDS while 2 * nbins of them fit
template <bool PLDA>
static hipError_t launch_histogram_tiles(const ScoreArgs& p, hipStream_t s) {
  int cus = 0;
  const hipError_t e = compute_units(&cus);
  if (e != hipSuccess) return e;
  const int64_t ntiles = (int64_t)p.nMt * p.nNt;
  const bool in_lds = p.nbins <= kScoreLdsBins;
  const size_t smem = kOperandBytes + kLabelBytes + (PLDA ? kBiasBytes : 0) + (in_lds ? (size_t)2 * p.nbins * sizeof(unsigned) : 0);
  const int per_cu = smem * 2 <= 160 * 1024 ? 2 : 1;
  int64_t grid = (int64_t)cus * per_cu;
  // a workgroup's LDS counters are 32 bits wide: at most 2^16 tiles of 2^14 scores each per workgroup
  if (in_lds && (ntiles + grid - 1) / grid > 65536) grid = (ntiles + 65535) / 65536;
  if (grid > ntiles) grid = ntiles;
  if (in_lds) return launch_tiles_v<PLDA ? EPI_PLDA_HIST_LDS : EPI_HIST_LDS>(p, (unsigned)grid, smem, s);
  return launch_tiles_v<PLDA ? EPI_PLDA_HIST_GLOBAL : EPI_HIST_GLOBAL>(p, (unsigned)grid, smem, s);
}

template <bool PLDA>
static hipError_t launch_pairs(const float* a, int64_t lda, int n, const float* row_bias, const float* b, int64_t ldb, int m,
                               const float* col_bias, int d, const int32_t* ia, const int32_t* ib, int64_t npairs, float* out,
                               hipStream_t s) {
  if (npairs <= 0) return hipSuccess;
  const auto kernel = ntg::nt_vec(a, lda, b, ldb) ? score_pairs_kernel<true, PLDA> : score_pairs_kernel<false, PLDA>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((npairs + 15) / 16)), dim3(256), 0, s, a, lda, n, b, ldb, m, d, ia, ib, npairs, out,
                     row_bias, col_bias);
  return hipGetLastError();
}

hipError_t launch_score_matrix(const float* a, int64_t lda, int n, const float* b, int64_t ldb, int m, int d,
                               const float* a_sub, int b_offset, float* out, int64_t ldo, hipStream_t s) {
  if (n <= 0 || m <= 0) return hipSuccess;
  ScoreArgs p = score_args(a, lda, n, b, ldb, m, d);
  p.C = out; p.ldc = ldo; p.a_sub = a_sub; p.b_offset = b_offset;
  return launch_matrix_tiles(p, false, s);
}

hipError_t launch_score_histogram(const float* a, int64_t lda, int n, const int32_t* la, const float* b, int64_t ldb, int m,
                                  const int32_t* lb, int d, int self, int nbins, unsigned long long* hs,
                                  unsigned long long* hd, hipStream_t s) {
  if (n <= 0 || m <= 0) return hipSuccess;
  ScoreArgs p = score_args(a, lda, n, b, ldb, m, d);
  p.la = la; p.lb = lb; p.self = self; p.nbins = nbins; p.hs = hs; p.hd = hd;
  return launch_histogram_tiles<false>(p, s);
}

hipError_t launch_score_pairs(const float* a, int64_t lda, int n, const float* b, int64_t ldb, int m, int d, const int32_t* ia,
                              const int32_t* ib, int64_t npairs, float* out, hipStream_t s) {
  return launch_pairs<false>(a, lda, n, nullptr, b, ldb, m, nullptr, d, ia, ib, npairs, out, s);
}

// ---------------------------------------------------------------------------------------------- PLDA launches
hipError_t launch_plda_rows(const float* u, int64_t ldu, int64_t rows, int d, int norm, int side, int pack_second,
                            const double* tables, const double* logdet, const int32_t* table_index, int num_tables,
                            float* rows_out, int64_t ldr, float* packed, int64_t ldp, float* bias, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(plda_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, u, ldu, rows, d, norm, side, pack_second,
                     tables, logdet, table_index, num_tables, rows_out, ldr, packed, ldp, bias);
  return hipGetLastError();
}

hipError_t launch_plda_matrix(const float* a, int64_t lda, int n, const float* row_bias, const float* b, int64_t ldb, int m,
                              const float* col_bias, int k, float* out, int64_t ldo, hipStream_t s) {
  if (n <= 0 || m <= 0) return hipSuccess;
  ScoreArgs p = score_args(a, lda, n, b, ldb, m, k);
  p.C = out; p.ldc = ldo; p.row_bias = row_bias; p.col_bias = col_bias;
  return launch_matrix_tiles(p, true, s);
}

hipError_t launch_plda_histogram(const float* a, int64_t lda, int n, const float* row_bias, const int32_t* la, const float* b,
                                 int64_t ldb, int m, const float* col_bias, const int32_t* lb, int k, double lo, double hi,
                                 int nbins, unsigned long long* hs, unsigned long long* hd, hipStream_t s) {
  if (n <= 0 || m <= 0) return hipSuccess;
  ScoreArgs p = score_args(a, lda, n, b, ldb, m, k);
  p.la = la; p.lb = lb; p.self = 0; p.nbins = nbins; p.hs = hs; p.hd = hd;
  p.row_bias = row_bias; p.col_bias = col_bias; p.lo = lo; p.bin_scale = (double)nbins / (hi - lo);
  return launch_histogram_tiles<true>(p, s);
}

hipError_t launch_plda_pairs(const float* a, int64_t lda, int n, const float* row_bias, const float* b, int64_t ldb, int m,
                             const float* col_bias, int k, const int32_t* ia, const int32_t* ib, int64_t npairs, float* out,
                             hipStream_t s) {
  return launch_pairs<true>(a, lda, n, row_bias, b, ldb, m, col_bias, k, ia, ib, npairs, out, s);
}

// ---------------------------------------------------------------------------------------------- panel launches
static int64_t cohort_panel_ld(int64_t m) { return m < 4 ? 4 : (m + 3) / 4 * 4; }

int64_t cohort_stats_workspace_bytes(int64_t n, int64_t m) {
  (void)n;                                       // one panel of SBM rows serves any n; more only means fewer launches
  return (int64_t)SBM * cohort_panel_ld(m) * (int64_t)sizeof(float);
}

int64_t score_topk_workspace_bytes(int64_t n, int64_t m) { return cohort_stats_workspace_bytes(n, m); }

// The panel walk of launch_cohort_stats and launch_score_topk: as many whole tile rows of scores as the workspace holds
// are written as a panel [rows, ldp] (rows padded to 4 floats), by the epilogue xv_score_matrix / xv_plda_matrix would use,
// so the panel holds the bits those calls would write; then select(panel, ldp, rows, r0, stage, sel_smem) launches one
// workgroup per panel row on rows r0 .. r0 + rows - 1, with the row staged in LDS (`stage`) when it fits.
template <typename Select>
static hipError_t walk_panels(const float* a, int64_t lda, int n, const float* row_bias, const float* b, int64_t ldb, int m,
                              const float* col_bias, int k, void* ws, int64_t ws_bytes, hipStream_t s, Select select) {
  if (n <= 0) return hipSuccess;
  const int64_t ldp = cohort_panel_ld(m);
  int64_t prows = ws_bytes / (ldp * (int64_t)sizeof(float)) / SBM * SBM;      // whole tile rows per panel
  const int64_t nceil = ((int64_t)n + SBM - 1) / SBM * SBM;
  if (prows > nceil) prows = nceil;
  if (prows < SBM) return hipErrorInvalidValue;                              // the caller checked ws_bytes
  float* panel = static_cast<float*>(ws);
  const bool stage = m <= kSelStageMax;
  const size_t sel_smem = kSelFixedBytes + (stage ? (size_t)m * sizeof(float) : 0);
  for (int64_t r0 = 0; r0 < n; r0 += prows) {
    const int rows = (int)(n - r0 < prows ? n - r0 : prows);
    if (m > 0) {
      ScoreArgs p = score_args(a + r0 * lda, lda, rows, b, ldb, m, k);
      p.C = panel; p.ldc = ldp;
      p.row_bias = row_bias ? row_bias + r0 : nullptr; p.col_bias = col_bias;
      const hipError_t e = launch_matrix_tiles(p, row_bias || col_bias, s);
      if (e != hipSuccess) return e;
    }
    select(panel, ldp, rows, r0, stage, sel_smem);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_cohort_stats(const float* a, int64_t lda, int n, const float* row_bias, const int32_t* la, const float* b,
                               int64_t ldb, int m, const float* col_bias, const int32_t* lb, int k, int top_k, float* mean,
                               float* stdv, int32_t* count, void* ws, int64_t ws_bytes, hipStream_t s) {
  return walk_panels(a, lda, n, row_bias, b, ldb, m, col_bias, k, ws, ws_bytes, s,
                     [&](const float* panel, int64_t ldp, int rows, int64_t r0, bool stage, size_t sel_smem) {
    const auto kernel = stage ? cohort_select_kernel<true> : cohort_select_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)rows), dim3(256), sel_smem, s, panel, ldp, m, la ? la + r0 : nullptr, lb, top_k,
                       mean + r0, stdv + r0, count ? count + r0 : nullptr);
  });
}

hipError_t launch_score_topk(const float* a, int64_t lda, int n, const float* row_bias, const int32_t* la, const float* b,
                             int64_t ldb, int m, const float* col_bias, const int32_t* lb, int k, int top_k, float* scores,
                             int32_t* index, int64_t ldo, int32_t* count, void* ws, int64_t ws_bytes, hipStream_t s) {
  const int vec = aligned16(ws) ? 1 : 0;         // panel rows are padded to 4 floats: 16-byte loads when the base allows
  return walk_panels(a, lda, n, row_bias, b, ldb, m, col_bias, k, ws, ws_bytes, s,
                     [&](const float* panel, int64_t ldp, int rows, int64_t r0, bool stage, size_t sel_smem) {
    const auto kernel = stage ? topk_select_kernel<true> : topk_select_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)rows), dim3(256), sel_smem, s, panel, ldp, m, la ? la + r0 : nullptr, lb, top_k,
                       scores + r0 * ldo, index + r0 * ldo, ldo, count ? count + r0 : nullptr, vec);
  });
}

}  // namespace xv
