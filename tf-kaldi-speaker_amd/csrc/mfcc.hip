// MFCC features and the energy VAD on the GPU: the first step of the reference recipe (egs/voxceleb/v1/run.sh:57-65),
//   steps/make_mfcc.sh --mfcc-config conf/mfcc.conf   (Kaldi compute-mfcc-feats)
//   sid/compute_vad_decision.sh                        (Kaldi compute-vad-decision)
// Kaldi is not part of the reference tree and the tree holds no conf/ directory; this restates the published algorithm.
// **parity unpinned** (no Kaldi binary or fixture available); checked against tests/helpers/ref_mfcc.py.
//
// Definition (option names and defaults are Kaldi's; samples are the int16 values as floats, no scaling to +-1):
//   frame options  --sample-frequency 16000, --frame-length 25 ms, --frame-shift 10 ms, --preemphasis-coefficient 0.97,
//                  --remove-dc-offset true, --window-type povey (hamming, hanning, rectangular), --round-to-power-of-two true
//                  (required here), --snip-edges true.  --dither: Kaldi's default 1.0 is random noise; here the default is 0
//                  and any other value is refused.
//   geometry       N = samples per frame, S = samples per shift, L = samples of the utterance.
//                  snip_edges:     T = 0 if L < N else 1 + (L - N) / S; frame t starts at t S.
//                  no snip_edges:  T = (L + S / 2) / S; frame t starts at t S + S / 2 - N / 2; an index outside [0, L) is
//                  reflected until it is inside: s < 0 -> -s - 1, s >= L -> 2 L - 1 - s.
//   per frame      1 subtract the frame mean; 2 raw log energy log(max(sum x^2, FLT_EPSILON)) (--raw-energy true: before
//                  pre-emphasis and window; false: after the window); 3 pre-emphasis x[i] -= c x[i-1], i = N-1..1, x[0] -= c x[0];
//                  4 window, povey = (0.5 - 0.5 cos(2 pi i / (N - 1)))^0.85; 5 zero-pad to the next power of two P; 6 real FFT;
//                  7 power spectrum of bins 0 .. P/2 - 1 (the mel bank does not use the Nyquist bin).
//   mel bank       --num-mel-bins 23, --low-freq 20, --high-freq 0 (<= 0: Nyquist + value); mel(f) = 1127 ln(1 + f / 700);
//                  M + 2 equally spaced mel points; weight of FFT bin i in filter m with u = mel(i fs / P) strictly inside
//                  (left, right): (u - left) / (centre - left) if u <= centre else (right - u) / (right - centre).  No VTLN.
//                  Mel energies are floored at FLT_EPSILON, then log.
//   cepstra        orthonormal DCT-II (row 0 sqrt(1/M), row k sqrt(2/M) cos(pi / M (n + 1/2) k)), first --num-ceps 13 rows,
//                  lifter 1 + Q/2 sin(pi k / Q) with --cepstral-lifter Q = 22; --use-energy true puts the log energy (floored
//                  at log(--energy-floor) when that is > 0) in coefficient 0.  --htk-compat is refused.
//   VAD            E = column 0; thr = --vad-energy-threshold 5.0 + --vad-energy-mean-scale 0.5 * mean(E); frame t is voiced
//                  iff #{u in [t-c, t+c] n [0, T): E[u] > thr} >= --vad-proportion-threshold 0.6 * #{u in that window},
//                  c = --vad-frames-context 0.  One float per frame, 0 or 1.
//
// Fbank (Kaldi compute-fbank-feats; steps/make_fbank.sh --fbank-config conf/fbank.conf of egs/voxceleb/v3/run.sh:54), also
// **parity unpinned**; checked against tests/helpers/ref_fbank.py.  The frame options, the steps 1-7 of a frame and the mel
// bank are the ones above; the pipeline stops after the mel sums, with three options of its own:
//   --use-power true       false: every power bin of step 7 is replaced by its square root before the mel sums.
//   --use-log-fbank true   mel energies are floored at FLT_EPSILON, then log; false: the mel energies are written as they are.
//   --use-energy false     true: the output has M + 1 columns and column 0 is the log energy of step 2 (--raw-energy as above,
//                          floored at log(--energy-floor) when that is > 0); false: M columns.
//   --num-mel-bins 23 (3..64).  --htk-compat, nonzero --dither and --round-to-power-of-two=false are refused as for the MFCC.
//   side output            the log energy of step 2 under this option set's --raw-energy and --energy-floor, one float per
//                          frame, whatever --use-energy says: what the energy VAD needs from a file that does not carry it.
//
// mfcc_kernel: a workgroup of four waves takes kRun consecutive frames of one utterance and loads the samples they share
// into LDS once (reflection applied there; consecutive frames overlap by 60 %).  Each wave then carries one frame at a time
// through every step in registers and its own LDS area; only the num_ceps outputs reach global memory.  The P-point real
// FFT is a P/2-point complex radix-2 FFT (decimation in frequency, natural order in, bit-reversed order out: the unpacking
// step reads through the bit reversal, so there is no permutation pass).  Every table (window, twiddles, mel weights with
// each filter's first bin and length, DCT x lifter) is built on the host in double and rounded once to fp32; the kernel
// calls no sin / cos / pow.  All arithmetic is fp32, every reduction has a fixed order, there are no atomics: two runs give
// the same bits.
// fbank_kernel: the same work split.  Both kernels take a tile through load_tile() and a frame through frame_power() -- samples
// to log energy and power spectrum, one set of statements -- so the side energy of fbank_kernel and coefficient 0 of
// mfcc_kernel with --use-energy are the same bits; fbank_kernel ends after mel_sum().
// LDS layout: stage twiddles are stored per stage, contiguously, so a butterfly stage reads them without bank conflicts;
// the butterflies themselves are conflict-free down to a span of 32 complex values and two-way below; the bit-reversed
// reads of the unpacking step are eight-way.  Left as is in this first version.
#include <cfloat>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/xvec_hip.h"
#include "xv_kernels.h"

namespace xv {

namespace {

constexpr int kRun = 16;          // frames per workgroup pass (four per wave)
constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr int kMaxMel = 64;

struct FrameParams {              // what both kernels need up to the mel sums
  int N, S, first_shift;          // samples per frame / per shift; start of frame 0 (0, or S/2 - N/2 without snip_edges)
  int M;                          // mel bins
  int remove_dc, raw_energy, use_energy;
  float preemph, log_energy_floor;        // log_energy_floor = -inf: none
  const float* window;            // [N]
  const float2* stage_tw;         // [H]: stage with half-span m at offset H - 2m, entry j = exp(-2 pi i j / (2m))
  const float2* unpack_tw;        // [H]: exp(-2 pi i k / P)
  const int32_t* mel_first;       // [M] first FFT bin of the filter
  const int32_t* mel_len;         // [M] bins of the filter
  const int32_t* mel_off;         // [M] offset of its weights in mel_w
  const float* mel_w;
};

struct MfccParams : FrameParams {
  int C;                          // cepstra
  const float* dct_t;             // [M, C]: dct_t[n * C + k] = lifter[k] * DCT[k][n]
  const float* dct_rowsum;        // [C]: sum_n of the above in double, rounded
};

struct FbankParams : FrameParams {
  int use_log, use_power;
};

__device__ __forceinline__ float wave_sum(float v) {     // fixed order: the same bits on every lane and every run
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// tile w of the launch belongs to utterance b iff base(b) <= w < base(b + 1), base(b) = off[b] / kRun + b: utterance b has
// ceil(T_b / kRun) <= base(b + 1) - base(b) runs; the at most one tile per utterance beyond that is idle.
__device__ __forceinline__ int tile_base(const int32_t* off, int b) { return off[b] / kRun + b; }

// Sum of the squares a lane holds, for the frame energy.  Its rounding is written out, not left to the compiler's choice between
// a multiply and an add or a fused multiply-add, which depends on the code around the loop: coefficient 0 of mfcc_kernel and the
// side energy of fbank_kernel have to be the same bits, and the bits mfcc_kernel gave before fbank_kernel shared its code.  With
// eight samples per lane (P = 512) every square is rounded and then added; with four (P = 256) the sum is one fused chain.
template <int K>
__device__ __forceinline__ float sum_squares(const float (&x)[K]) {
  if constexpr (K == 8) {
#pragma clang fp contract(off)
    float e = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) e += x[k] * x[k];
    return e;
  } else {
    float e = x[0] * x[0];
#pragma unroll
    for (int k = 1; k < K; ++k) e = __builtin_fmaf(x[k], x[k], e);
    return e;
  }
}

// Finds the utterance and the run of frames of tile w and loads the samples those frames share into `span`, reflection applied.
// Returns false for an idle tile; otherwise row0 is the output row of the tile's first frame and nf its frame count.  Every
// branch is uniform over the workgroup.
__device__ __forceinline__ bool load_tile(const FrameParams& p, const int16_t* __restrict__ wave, const int64_t* __restrict__ soff,
                                          const int32_t* __restrict__ foff, int B, int w, float* span, int64_t& row0, int& nf) {
  const int tid = threadIdx.x;
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tile_base(foff, mid) <= w) lo = mid; else hi = mid - 1;
  }
  const int b = lo;
  const int T = foff[b + 1] - foff[b];
  const int t0 = (w - tile_base(foff, b)) * kRun;
  const int64_t L = soff[b + 1] - soff[b];
  if (t0 >= T || L <= 0) return false;
  nf = min(kRun, T - t0);
  row0 = (int64_t)foff[b] + t0;
  const int64_t first = (int64_t)t0 * p.S + p.first_shift;
  const int span_len = (nf - 1) * p.S + p.N;
  __syncthreads();                                           // the previous tile has been read (and the tables are in)
  const int16_t* src = wave + soff[b];
  for (int j = tid; j < span_len; j += kThreads) {
    int64_t s = first + j;
    while (s < 0 || s >= L) s = (s < 0) ? -s - 1 : 2 * L - 1 - s;
    span[j] = (float)src[s];
  }
  __syncthreads();
  return true;
}

// Steps 1-7 of a frame on one wave: the N samples at x0 -> the (floored) log energy, returned on every lane, and the power
// spectrum (its square root with `amplitude`) of bins 0 .. P/2 - 1 in pw.  z [P] and pw [P/2] are this wave's LDS areas.  All
// four waves call it together: it holds workgroup barriers, the last one after pw is complete.
template <int P>
__device__ __forceinline__ float frame_power(const FrameParams& p, bool amplitude, const float* x0, float* z, float* pw,
                                             const float2* stage_tw, const float2* unpack_tw, int lane) {
  constexpr int H = P / 2;                 // complex FFT length
  constexpr int K = P / 64;                // samples per lane
  constexpr int LOG2H = (P == 512) ? 8 : 7;
  float2* cz = reinterpret_cast<float2*>(z);
  float x[K], xp[K];
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int i = lane + 64 * k;
    x[k] = i < p.N ? x0[i] : 0.f;
    xp[k] = i < p.N ? x0[max(i - 1, 0)] : 0.f;
    sum += x[k];
  }
  if (p.remove_dc) {
    const float mean = wave_sum(sum) / (float)p.N;
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (lane + 64 * k < p.N) { x[k] -= mean; xp[k] -= mean; }
  }
  float e = 0.f;
  if (p.raw_energy) e = sum_squares(x);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int i = lane + 64 * k;
    x[k] = i < p.N ? (x[k] - p.preemph * xp[k]) * p.window[i] : 0.f;
    z[i] = x[k];
  }
  if (!p.raw_energy) e = sum_squares(x);
  float log_e = logf(fmaxf(wave_sum(e), FLT_EPSILON));
  log_e = fmaxf(log_e, p.log_energy_floor);
  __syncthreads();

  // H-point complex FFT of cz[j] = z[2j] + i z[2j+1], decimation in frequency
#pragma unroll
  for (int m = H / 2; m >= 1; m >>= 1) {
    const float2* tw = stage_tw + (H - 2 * m);
#pragma unroll
    for (int q = lane; q < H / 2; q += 64) {
      const int j = q & (m - 1);
      const int a = ((q - j) << 1) + j;
      const float2 u = cz[a], v = cz[a + m], t = tw[j];
      const float dr = u.x - v.x, di = u.y - v.y;
      cz[a] = make_float2(u.x + v.x, u.y + v.y);
      cz[a + m] = make_float2(dr * t.x - di * t.y, dr * t.y + di * t.x);
    }
    __syncthreads();
  }
  // unpack to the real transform: X[k] = E[k] + W_P^k O[k], E = (Z[k] + conj Z[H-k]) / 2, O = -i (Z[k] - conj Z[H-k]) / 2
#pragma unroll
  for (int k = lane; k < H; k += 64) {
    const float2 zk = cz[__brev((unsigned)k) >> (32 - LOG2H)];
    const float2 zn = cz[__brev((unsigned)((H - k) & (H - 1))) >> (32 - LOG2H)];
    const float er = 0.5f * (zk.x + zn.x), ei = 0.5f * (zk.y - zn.y);
    const float orr = 0.5f * (zk.y + zn.y), oi = -0.5f * (zk.x - zn.x);
    const float2 t = unpack_tw[k];
    const float xr = er + (t.x * orr - t.y * oi), xi = ei + (t.x * oi + t.y * orr);
    const float pk = xr * xr + xi * xi;
    pw[k] = amplitude ? sqrtf(pk) : pk;
  }
  __syncthreads();
  return log_e;
}

// mel energy of filter `lane` (< M), before the floor and the log
__device__ __forceinline__ float mel_sum(const FrameParams& p, const float* pw, int lane) {
  const int fb = p.mel_first[lane], n = p.mel_len[lane];
  const float* wgt = p.mel_w + p.mel_off[lane];
  float acc = 0.f;
  for (int i = 0; i < n; ++i) acc += wgt[i] * pw[fb + i];
  return acc;
}

template <int P>
__global__ __launch_bounds__(kThreads) void mfcc_kernel(MfccParams p, const int16_t* __restrict__ wave,
                                                        const int64_t* __restrict__ soff, const int32_t* __restrict__ foff,
                                                        int B, float* __restrict__ out, int64_t ld) {
  constexpr int H = P / 2;
  extern __shared__ __align__(16) float lds[];
  float2* stage_tw = reinterpret_cast<float2*>(lds);          // [H]
  float2* unpack_tw = stage_tw + H;                            // [H]
  float* area = lds + 4 * H;                                   // per wave: z [P] | power [H] | mel [kMaxMel]
  constexpr int kArea = P + H + kMaxMel;
  float* span = area + kWaves * kArea;                         // [(kRun - 1) S + N]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float* z = area + wv * kArea;
  float* pw = z + P;
  float* melbuf = pw + H;

  for (int i = tid; i < H; i += kThreads) {
    stage_tw[i] = p.stage_tw[i];
    unpack_tw[i] = p.unpack_tw[i];
  }
  const int tiles = foff[B] / kRun + B;
  for (int w = blockIdx.x; w < tiles; w += gridDim.x) {
    int64_t row0;
    int nf;
    if (!load_tile(p, wave, soff, foff, B, w, span, row0, nf)) continue;
    for (int it = 0; it < kRun / kWaves; ++it) {
      const int f = it * kWaves + wv;
      const bool valid = f < nf;
      const float log_e = frame_power<P>(p, false, span + (valid ? f * p.S : 0), z, pw, stage_tw, unpack_tw, lane);
      if (lane < p.M) melbuf[lane] = logf(fmaxf(mel_sum(p, pw, lane), FLT_EPSILON));
      __syncthreads();
      if (lane < p.C) {
        // sum_n D[k][n] mel[n] = sum_n D[k][n] (mel[n] - c) + c sum_n D[k][n]: the second sum is known in double (it is
        // sqrt(M) for row 0 and 0 for the others), so the cancellation of a flat spectrum costs no accuracy
        const float c = melbuf[0];
        float acc = 0.f;
        for (int n = 1; n < p.M; ++n) acc += p.dct_t[n * p.C + lane] * (melbuf[n] - c);
        acc += p.dct_rowsum[lane] * c;
        if (lane == 0 && p.use_energy) acc = log_e;
        if (valid) out[(row0 + f) * ld + lane] = acc;
      }
    }
  }
}

// compute-fbank-feats: as mfcc_kernel up to the mel sums.  Lanes < M write column lane + use_energy, lane 0 the energy column
// and the side energy (log_energy may be null).  The per-wave LDS areas are only written again behind the barriers of the
// next frame_power(), so no barrier follows the mel sums.
template <int P>
__global__ __launch_bounds__(kThreads) void fbank_kernel(FbankParams p, const int16_t* __restrict__ wave,
                                                         const int64_t* __restrict__ soff, const int32_t* __restrict__ foff,
                                                         int B, float* __restrict__ out, int64_t ld, float* __restrict__ log_energy) {
  constexpr int H = P / 2;
  extern __shared__ __align__(16) float lds[];
  float2* stage_tw = reinterpret_cast<float2*>(lds);          // [H]
  float2* unpack_tw = stage_tw + H;                            // [H]
  float* area = lds + 4 * H;                                   // per wave: z [P] | power [H]
  constexpr int kArea = P + H;
  float* span = area + kWaves * kArea;                         // [(kRun - 1) S + N]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float* z = area + wv * kArea;
  float* pw = z + P;

  for (int i = tid; i < H; i += kThreads) {
    stage_tw[i] = p.stage_tw[i];
    unpack_tw[i] = p.unpack_tw[i];
  }
  const int tiles = foff[B] / kRun + B;
  for (int w = blockIdx.x; w < tiles; w += gridDim.x) {
    int64_t row0;
    int nf;
    if (!load_tile(p, wave, soff, foff, B, w, span, row0, nf)) continue;
    for (int it = 0; it < kRun / kWaves; ++it) {
      const int f = it * kWaves + wv;
      const bool valid = f < nf;
      const float log_e = frame_power<P>(p, !p.use_power, span + (valid ? f * p.S : 0), z, pw, stage_tw, unpack_tw, lane);
      if (lane < p.M) {
        float acc = mel_sum(p, pw, lane);
        if (p.use_log) acc = logf(fmaxf(acc, FLT_EPSILON));
        if (valid) out[(row0 + f) * ld + lane + p.use_energy] = acc;
      }
      if (lane == 0 && valid) {
        if (p.use_energy) out[(row0 + f) * ld] = log_e;
        if (log_energy) log_energy[row0 + f] = log_e;
      }
    }
  }
}

// one workgroup per utterance.  Pass 1: mean of E = feats[:, 0] in double, fixed order (per-thread strided partial sums, then a
// tree over the workgroup).  Pass 2: one thread per frame counts the frames above the threshold in its clipped window.
__global__ __launch_bounds__(256) void vad_kernel(const float* __restrict__ feats, int64_t ld, const int32_t* __restrict__ foff,
                                                  float threshold, float mean_scale, int context, float proportion,
                                                  float* __restrict__ vad) {
  __shared__ double part[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int r0 = foff[b], T = foff[b + 1] - r0;
  if (T <= 0) return;
  const float* E = feats + (int64_t)r0 * ld;
  double s = 0.0;
  for (int t = tid; t < T; t += 256) s += (double)E[(int64_t)t * ld];
  part[tid] = s;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) part[tid] += part[tid + o];
    __syncthreads();
  }
  const double thr = (double)threshold + (double)mean_scale * (part[0] / (double)T);
  for (int t = tid; t < T; t += 256) {
    const int u0 = max(t - context, 0), u1 = min(t + context, T - 1);
    int num = 0;
    for (int u = u0; u <= u1; ++u) num += ((double)E[(int64_t)u * ld] > thr) ? 1 : 0;
    const float need = (float)(u1 - u0 + 1) * proportion;        // Kaldi compares in float
    vad[r0 + t] = ((float)num >= need) ? 1.f : 0.f;
  }
}

double mel_scale(double f) { return 1127.0 * std::log(1.0 + f / 700.0); }

template <class T>
hipError_t upload(const std::vector<T>& v, void** dev) {
  *dev = nullptr;
  hipError_t e = hipMalloc(dev, std::max<size_t>(v.size(), 1) * sizeof(T));
  if (e != hipSuccess) return e;
  return hipMemcpy(*dev, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

struct FrontTables {              // host side of FrameParams: sizes and the tables both feature types share
  int N = 0, S = 0, P = 0;
  std::vector<float> window;
  std::vector<float2> stage_tw, unpack_tw;
  std::vector<int32_t> mel_first, mel_len, mel_off;
  std::vector<float> mel_w;
};

struct FrontHandle {              // what xv_mfcc and xv_fbank have in common
  int P = 0;
  int device = 0;
  int snip_edges = 1;
  int grid = 0;
  size_t lds_bytes = 0;
  std::vector<void*> bufs;
  ~FrontHandle() {
    for (void* b : bufs)
      if (b) (void)hipFree(b);
  }
};

// The checks of the options compute-mfcc-feats and compute-fbank-feats share (O is xv_mfcc_opts or xv_fbank_opts), then the
// shared tables.  No HIP call.
template <class O>
int front_tables(const O* o, FrontTables* t, std::string* err) {
  const double kPi = 3.14159265358979323846;
  auto bad = [&](int code, const std::string& m) { *err = m; return code; };
  if (o->dither != 0.f)
    return bad(XV_ERR_UNSUPPORTED, "--dither must be 0: random dither (Kaldi's default 1.0) is not implemented, features are deterministic");
  if (o->htk_compat) return bad(XV_ERR_UNSUPPORTED, "--htk-compat is not supported");
  if (!(o->sample_frequency > 0.f) || !(o->frame_length_ms > 0.f) || !(o->frame_shift_ms > 0.f))
    return bad(XV_ERR_INVALID, "--sample-frequency, --frame-length and --frame-shift must be positive");
  const int N = (int)((double)o->sample_frequency * 0.001 * (double)o->frame_length_ms);     // Kaldi: double, truncated
  const int S = (int)((double)o->sample_frequency * 0.001 * (double)o->frame_shift_ms);
  if (N < 2 || S < 1 || S > N) return bad(XV_ERR_UNSUPPORTED, "frame length must be at least 2 samples and the frame shift between 1 sample and the frame length");
  if (!o->round_to_power_of_two) return bad(XV_ERR_UNSUPPORTED, "--round-to-power-of-two=false is not supported");
  int P = 1;
  while (P < N) P <<= 1;
  if (P != 256 && P != 512)
    return bad(XV_ERR_UNSUPPORTED, "padded frame length " + std::to_string(P) + " is not supported (256 and 512 are: 129..512 samples per frame)");
  const int M = o->num_mel_bins;
  if (M < 3 || M > kMaxMel) return bad(XV_ERR_UNSUPPORTED, "--num-mel-bins must be between 3 and 64");
  if (o->window_type < XV_WINDOW_POVEY || o->window_type > XV_WINDOW_RECTANGULAR) return bad(XV_ERR_INVALID, "unknown --window-type");
  if (o->preemphasis_coefficient < 0.f || o->preemphasis_coefficient > 1.f) return bad(XV_ERR_INVALID, "--preemphasis-coefficient must be in [0, 1]");
  const double fs = o->sample_frequency, nyquist = 0.5 * fs;
  const double low = o->low_freq, high = o->high_freq > 0.f ? (double)o->high_freq : nyquist + (double)o->high_freq;
  if (low < 0.0 || low >= nyquist || high <= 0.0 || high > nyquist || high <= low)
    return bad(XV_ERR_INVALID, "bad --low-freq / --high-freq for this sample frequency");

  const int H = P / 2;
  t->N = N; t->S = S; t->P = P;
  t->window.resize(N);
  for (int i = 0; i < N; ++i) {
    const double a = 2.0 * kPi * i / (N - 1);
    double w = 1.0;
    if (o->window_type == XV_WINDOW_POVEY) w = std::pow(0.5 - 0.5 * std::cos(a), 0.85);
    else if (o->window_type == XV_WINDOW_HAMMING) w = 0.54 - 0.46 * std::cos(a);
    else if (o->window_type == XV_WINDOW_HANNING) w = 0.5 - 0.5 * std::cos(a);
    t->window[i] = (float)w;
  }
  t->stage_tw.resize(H);
  t->unpack_tw.resize(H);
  t->stage_tw[H - 1] = make_float2(0.f, 0.f);                   // unused pad
  for (int m = H / 2; m >= 1; m >>= 1)
    for (int j = 0; j < m; ++j) {
      const double a = -2.0 * kPi * j / (2.0 * m);
      t->stage_tw[H - 2 * m + j] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
  for (int k = 0; k < H; ++k) {
    const double a = -2.0 * kPi * k / P;
    t->unpack_tw[k] = make_float2((float)std::cos(a), (float)std::sin(a));
  }
  t->mel_first.resize(M);
  t->mel_len.resize(M);
  t->mel_off.resize(M);
  const double mel_low = mel_scale(low), mel_high = mel_scale(high), delta = (mel_high - mel_low) / (M + 1);
  for (int m = 0; m < M; ++m) {
    const double left = mel_low + m * delta, centre = mel_low + (m + 1) * delta, right = mel_low + (m + 2) * delta;
    int fb = -1, lb = -2;
    std::vector<double> wrow(H, 0.0);
    for (int i = 0; i < H; ++i) {
      const double u = mel_scale(fs / P * i);
      if (u > left && u < right) {
        wrow[i] = u <= centre ? (u - left) / (centre - left) : (right - u) / (right - centre);
        if (fb < 0) fb = i;
        lb = i;
      }
    }
    t->mel_first[m] = fb < 0 ? 0 : fb;
    t->mel_len[m] = fb < 0 ? 0 : lb - fb + 1;
    t->mel_off[m] = (int32_t)t->mel_w.size();
    for (int i = 0; i < t->mel_len[m]; ++i) t->mel_w.push_back((float)wrow[fb + i]);
  }
  return XV_OK;
}

// Uploads the shared tables (bufs 0..6) and `extra` (bufs 7..) to `device` and fills the handle and the shared kernel parameters.
template <class O>
hipError_t front_upload(const O* o, const FrontTables& t, const std::vector<const std::vector<float>*>& extra, int device,
                        FrontHandle* h, FrameParams* p) {
  int prev = -1;
  hipError_t e = hipGetDevice(&prev);
  if (e == hipSuccess && prev != device) e = hipSetDevice(device);
  if (e != hipSuccess) return e;
  h->P = t.P;
  h->device = device;
  h->snip_edges = o->snip_edges ? 1 : 0;
  p->N = t.N; p->S = t.S; p->first_shift = o->snip_edges ? 0 : t.S / 2 - t.N / 2;
  p->M = o->num_mel_bins;
  p->remove_dc = o->remove_dc_offset ? 1 : 0;
  p->raw_energy = o->raw_energy ? 1 : 0;
  p->use_energy = o->use_energy ? 1 : 0;
  p->preemph = o->preemphasis_coefficient;
  p->log_energy_floor = o->energy_floor > 0.f ? (float)std::log((double)o->energy_floor) : -INFINITY;
  h->bufs.resize(7 + extra.size(), nullptr);
  e = upload(t.window, &h->bufs[0]);
  if (e == hipSuccess) e = upload(t.stage_tw, &h->bufs[1]);
  if (e == hipSuccess) e = upload(t.unpack_tw, &h->bufs[2]);
  if (e == hipSuccess) e = upload(t.mel_first, &h->bufs[3]);
  if (e == hipSuccess) e = upload(t.mel_len, &h->bufs[4]);
  if (e == hipSuccess) e = upload(t.mel_off, &h->bufs[5]);
  if (e == hipSuccess) e = upload(t.mel_w, &h->bufs[6]);
  for (size_t i = 0; i < extra.size() && e == hipSuccess; ++i) e = upload(*extra[i], &h->bufs[7 + i]);
  hipDeviceProp_t prop;
  if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device);
  if (prev != device) (void)hipSetDevice(prev);
  if (e != hipSuccess) return e;
  p->window = (const float*)h->bufs[0];
  p->stage_tw = (const float2*)h->bufs[1];
  p->unpack_tw = (const float2*)h->bufs[2];
  p->mel_first = (const int32_t*)h->bufs[3];
  p->mel_len = (const int32_t*)h->bufs[4];
  p->mel_off = (const int32_t*)h->bufs[5];
  p->mel_w = (const float*)h->bufs[6];
  h->grid = std::max(prop.multiProcessorCount, 1) * 8;
  return hipSuccess;
}

int front_num_frames(const FrontHandle* h, const FrameParams& p, int64_t L, int64_t* out) {
  if (L < 0) return -1;
  *out = h->snip_edges ? (L < p.N ? 0 : 1 + (L - p.N) / p.S) : (L + p.S / 2) / p.S;
  return 0;
}

}  // namespace

}  // namespace xv

struct xv_mfcc : xv::FrontHandle {
  xv::MfccParams p;
};

struct xv_fbank : xv::FrontHandle {
  xv::FbankParams p;
};

namespace xv {

int mfcc_num_frames(const xv_mfcc* h, int64_t L, int64_t* out) { return front_num_frames(h, h->p, L, out); }

void mfcc_destroy(xv_mfcc* h) { delete h; }

// Validates the options and builds the tables.  Returns XV_OK or an XV_ERR_* code with the reason in `err`; every option check
// comes before the first HIP call.
int mfcc_create(const xv_mfcc_opts* o, int device, xv_mfcc** out, std::string* err) {
  const double kPi = 3.14159265358979323846;
  auto bad = [&](int code, const std::string& m) { *err = m; return code; };
  if (o->struct_size != (int32_t)sizeof(xv_mfcc_opts)) return bad(XV_ERR_INVALID, "xv_mfcc_opts.struct_size does not match this library");
  FrontTables t;
  const int rc = front_tables(o, &t, err);
  if (rc != XV_OK) return rc;
  const int M = o->num_mel_bins, C = o->num_ceps;
  if (C < 1 || C > M) return bad(XV_ERR_INVALID, "--num-ceps must be between 1 and --num-mel-bins");
  if (o->cepstral_lifter < 0.f) return bad(XV_ERR_INVALID, "--cepstral-lifter must not be negative");
  std::vector<float> dct_t((size_t)M * C), rowsum(C);
  for (int k = 0; k < C; ++k) {
    const double Q = o->cepstral_lifter;
    const double lift = Q > 0.0 ? 1.0 + 0.5 * Q * std::sin(kPi * k / Q) : 1.0;
    double sum = 0.0;
    for (int n = 0; n < M; ++n) {
      const double d = (k == 0 ? std::sqrt(1.0 / M) : std::sqrt(2.0 / M) * std::cos(kPi / M * (n + 0.5) * k)) * lift;
      dct_t[(size_t)n * C + k] = (float)d;
      sum += d;
    }
    rowsum[k] = (float)sum;
  }

  xv_mfcc* h = new xv_mfcc();
  const hipError_t e = front_upload(o, t, {&dct_t, &rowsum}, device, h, &h->p);
  if (e != hipSuccess) {
    delete h;
    return bad(XV_ERR_HIP, std::string("MFCC table upload to HIP device ") + std::to_string(device) + " failed: " + hipGetErrorString(e));
  }
  h->p.C = C;
  h->p.dct_t = (const float*)h->bufs[7];
  h->p.dct_rowsum = (const float*)h->bufs[8];
  const int H = t.P / 2;
  h->lds_bytes = sizeof(float) * (size_t)(4 * H + kWaves * (t.P + H + kMaxMel) + (kRun - 1) * t.S + t.N);   // <= 49 KiB (N = S = 512: 12544 floats)
  *out = h;
  return XV_OK;
}

int mfcc_device(const xv_mfcc* h) { return h->device; }

hipError_t launch_mfcc(xv_mfcc* h, const int16_t* wave, const int64_t* soff, const int32_t* foff, int B, float* out,
                       int64_t ld, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (h->P == 512)
    hipLaunchKernelGGL(mfcc_kernel<512>, dim3(h->grid), dim3(kThreads), h->lds_bytes, s, h->p, wave, soff, foff, B, out, ld);
  else
    hipLaunchKernelGGL(mfcc_kernel<256>, dim3(h->grid), dim3(kThreads), h->lds_bytes, s, h->p, wave, soff, foff, B, out, ld);
  return hipGetLastError();
}

int mfcc_num_ceps(const xv_mfcc* h) { return h->p.C; }

int fbank_num_frames(const xv_fbank* h, int64_t L, int64_t* out) { return front_num_frames(h, h->p, L, out); }

void fbank_destroy(xv_fbank* h) { delete h; }

int fbank_create(const xv_fbank_opts* o, int device, xv_fbank** out, std::string* err) {
  auto bad = [&](int code, const std::string& m) { *err = m; return code; };
  if (o->struct_size != (int32_t)sizeof(xv_fbank_opts)) return bad(XV_ERR_INVALID, "xv_fbank_opts.struct_size does not match this library");
  FrontTables t;
  const int rc = front_tables(o, &t, err);
  if (rc != XV_OK) return rc;
  xv_fbank* h = new xv_fbank();
  const hipError_t e = front_upload(o, t, {}, device, h, &h->p);
  if (e != hipSuccess) {
    delete h;
    return bad(XV_ERR_HIP, std::string("fbank table upload to HIP device ") + std::to_string(device) + " failed: " + hipGetErrorString(e));
  }
  h->p.use_log = o->use_log_fbank ? 1 : 0;
  h->p.use_power = o->use_power ? 1 : 0;
  const int H = t.P / 2;
  h->lds_bytes = sizeof(float) * (size_t)(4 * H + kWaves * (t.P + H) + (kRun - 1) * t.S + t.N);             // <= 48 KiB (N = S = 512: 12288 floats)
  *out = h;
  return XV_OK;
}

int fbank_device(const xv_fbank* h) { return h->device; }

int fbank_num_feats(const xv_fbank* h) { return h->p.M + h->p.use_energy; }

hipError_t launch_fbank(xv_fbank* h, const int16_t* wave, const int64_t* soff, const int32_t* foff, int B, float* out,
                        int64_t ld, float* log_energy, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (h->P == 512)
    hipLaunchKernelGGL(fbank_kernel<512>, dim3(h->grid), dim3(kThreads), h->lds_bytes, s, h->p, wave, soff, foff, B, out, ld,
                       log_energy);
  else
    hipLaunchKernelGGL(fbank_kernel<256>, dim3(h->grid), dim3(kThreads), h->lds_bytes, s, h->p, wave, soff, foff, B, out, ld,
                       log_energy);
  return hipGetLastError();
}

hipError_t launch_vad_energy(const float* feats, int64_t ld, const int32_t* foff, int B, float threshold, float mean_scale,
                             int context, float proportion, float* vad, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(vad_kernel, dim3(B), dim3(256), 0, s, feats, ld, foff, threshold, mean_scale, context, proportion, vad);
  return hipGetLastError();
}

}  // namespace xv
