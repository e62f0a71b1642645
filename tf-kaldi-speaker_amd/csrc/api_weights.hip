// C ABI of libxvec_hip.so, the weights: xv_finalize chooses each layer's kernel and number format, folds the batch
// normalisation and packs the weights into the layouts the gfx950 kernels read; the fp16 range flags.
#include "layer_lines.h"
#include "xv_model.h"

using namespace xv;
using namespace xv::api;

namespace {

using lines::kBnEps;                   // the one epsilon of the training layers too

uint16_t f32_to_bf16_rn(float f) {   // round to nearest even; inputs are finite weights
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
float bf16_to_f32(uint16_t b) {
  uint32_t u = (uint32_t)b << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
uint16_t f32_to_f16_rn(float f) {    // IEEE binary16, round to nearest even (subnormals kept, overflow -> inf)
  const _Float16 h = (_Float16)f;
  uint16_t u;
  memcpy(&u, &h, 2);
  return u;
}
float f16_to_f32(uint16_t u) {
  _Float16 h;
  memcpy(&h, &u, 2);
  return (float)h;
}

const HostTensor& T(const xv_handle* h, const std::string& n) { return h->tensors.at(n); }

// s = gamma / sqrt(var + eps), t = beta - mean * s   (inference BN as one multiply-add)
void bn_fold(const xv_handle* h, const std::string& scope, int n, std::vector<double>& s, std::vector<double>& t) {
  const auto& g = T(h, scope + "/gamma").data;
  const auto& b = T(h, scope + "/beta").data;
  const auto& m = T(h, scope + "/moving_mean").data;
  const auto& v = T(h, scope + "/moving_variance").data;
  s.resize(n); t.resize(n);
  for (int i = 0; i < n; ++i) {
    s[i] = (double)g[i] / std::sqrt((double)v[i] + kBnEps);
    t[i] = (double)b[i] - (double)m[i] * s[i];
  }
}

// ---- block-scaled fp6 (e2m3) quantisation of 32 values: the host twin of e2m3_code / e8m0_of in csrc/gemm_f16f6.hip
uint32_t host_e2m3(float x, float inv) {
  float v = std::fmin(std::fabs(x) * inv, 7.5f);
  const bool sub = v < 1.f;
  const float t = sub ? v + 1.f : v;
  uint32_t bits;
  memcpy(&bits, &t, 4);
  uint32_t c = ((bits + 0x80000u) >> 20) - (126u << 3) - (sub ? 8u : 0u);
  c = c > 31u ? 31u : c;
  return c | (x < 0.f ? 32u : 0u);
}
void host_quant32(const float* v, unsigned char* codes24, unsigned char* scale_byte) {
  float amax = 0.f;
  for (int i = 0; i < 32; ++i) amax = std::fmax(amax, std::fabs(v[i]));
  float inv = 1.f;
  uint32_t byte = 0;
  if (amax > 0.f && std::isfinite(amax)) {
    const float r = amax * (1.f / 7.5f);
    uint32_t bits;
    memcpy(&bits, &r, 4);
    int e = (int)((bits + 0x7FFFFFu) >> 23) - 127;
    e = e < -126 ? -126 : (e > 126 ? 126 : e);
    byte = (uint32_t)(127 + e);
    const uint32_t ib = (uint32_t)(127 - e) << 23;
    memcpy(&inv, &ib, 4);
  }
  memset(codes24, 0, 24);
  for (int i = 0; i < 32; ++i) {
    const uint32_t c = host_e2m3(v[i], inv);
    const int bit = 6 * i;
    for (int q = 0; q < 6; ++q)
      if ((c >> q) & 1) codes24[(bit + q) >> 3] |= (unsigned char)(1u << ((bit + q) & 7));
  }
  *scale_byte = (unsigned char)byte;
}

// fp16 split formats (XV_PREC_F16X3 / F16F6): power of two the split copy of a layer's output is kept at.  hi + lo carries 22
// significand bits only while the low half is a normal fp16 number (|x| >= 2^-3); below that it goes subnormal, and a layer whose
// activations sit around 1e-3 would lose precision silently (there is a flag for the other end of the range, none for this one).
// Behind a batch normalisation the pre-activation output of channel c is ~ N(beta_c, gamma_c^2) -- that is what the normalisation
// is for -- so the layer's rms is known from the weights: the split copy holds y * 2^e with rms * 2^e ~ 2^4 (values below 2^-3 are
// then < 1 % of the rms, four orders of magnitude of headroom to 65504 remain), and the reader's per-channel scale takes 2^-e
// (exact).  Layers without a normalisation, and tanh (not homogeneous, bounded anyway), keep e = 0.
int act_exponent(const xv_handle* h, const Layer& L) {
  if (!L.has_bn || L.act == ACT_TANH) return 0;
  const auto& g = T(h, L.bn_scope + "/gamma").data;
  const auto& b = T(h, L.bn_scope + "/beta").data;
  double s = 0.0;
  for (size_t i = 0; i < g.size(); ++i) s += (double)g[i] * g[i] + (double)b[i] * b[i];
  const double rms = std::sqrt(s / std::max<size_t>(g.size(), 1));
  if (!(rms > 0.0) || !std::isfinite(rms)) return 0;
  return (int)std::min(20.0, std::max(-20.0, std::floor(4.5 - std::log2(rms))));
}

// XV_PREC_F16F6: can the two-unit kernel hold this layer?  Its cross terms are fp6 under ONE power-of-two scale per 32 channels along
// K -- per (frame, block) for the activations, per (block, tap, output column) for the weights -- so a channel much smaller than the
// largest of its block is quantised against that largest value, and its cross terms fall towards plain fp16 (2^-11).  A trained
// model may put exactly that into a block (magnitude split between a BN scale and the next kernel's rows).  Estimate, from numbers
// known here, how much larger the block-scale error is than for channels of equal magnitude:
//   m_c  = expected magnitude of input channel c = sqrt(s_c^2 + shift_c^2) of the producer's folded BN (1 when unknown: no BN,
//          a residual sum, a pooling or the network input),
//   r_a  = sqrt(sum_c M_b(c)^2 W_c^2 / sum_c m_c^2 W_c^2)    M_b(c) = largest m of c's block, W_c^2 = sum over taps, columns of w^2,
//   r_w  = sqrt(sum_(c,tap,n) m_c^2 Wmax^2 / sum m_c^2 w^2)  Wmax = largest |w| of the (block, tap, n) K group of w,
// and demote the layer (f16x3 kernels, as for channel counts without a quad of blocks) when hypot(r_a, r_w) > kF6MaxSpread.
// A heuristic, with assumptions no test breaks: m_c takes the pre-BN output at unit variance (a channel whose real variance differs
// from moving_variance is misjudged either way) and ignores the activation behind the BN (a mostly dead ReLU channel, shift far
// below -s, is much smaller than m_c says, so spread of that kind is underestimated).  Calibrated
// with the CPU emulation (tests/analysis/f16f8_error_model.py, tests/test_f6_error_model.py): ~2.4 on every synthetic model (frame-level
// error 1.1e-5 .. 1.5e-5 against the exact path), 11 for a compensated per-channel spread of 2^+-2 (2.6e-5), 35 for 2^+-3 (6.5e-5,
// beyond the 5e-5 the two-unit layers are held to), 110 for 2^+-4 (1.5e-4).
constexpr double kF6MaxSpread = 16.0;

double f6_block_spread(const xv_handle* h, const Op& op, const Layer& L) {
  const int fw = L.mode == 1 ? 3 : L.w, fcin = L.mode == 1 ? 3 * L.cin : L.cin, N = L.cout, nb = fcin / 32;
  std::vector<double> m((size_t)fcin, 1.0);
  for (const Op& p : h->ops) {
    if (p.kind != OP_GEMM || p.out != op.in0 || p.in1 > 0) continue;
    const Layer& P = h->layers[p.layer];
    if (!P.has_bn || P.cout != L.cin) break;
    std::vector<double> s, t;
    bn_fold(h, P.bn_scope, P.cout, s, t);
    const auto* bias = P.has_bias ? &T(h, P.bias_name).data : nullptr;
    for (int r = 0; r < fcin; ++r) {
      const int c = r % L.cin;                       // grid convolution: kernel row kf * cin + c reads channel c
      const double sh = (bias ? (double)(*bias)[c] * s[c] : 0.0) + t[c];
      m[r] = std::sqrt(s[c] * s[c] + sh * sh);
    }
    break;
  }
  const auto& W = T(h, L.kernel_name).data;          // row (tap * fcin + r), column n
  std::vector<double> w2((size_t)fcin, 0.0);
  double num_w = 0.0, den = 0.0;
  for (int j = 0; j < fw; ++j)
    for (int b = 0; b < nb; ++b)
      for (int n = 0; n < N; ++n) {
        double wmax = 0.0, m2 = 0.0;
        for (int t = 0; t < 32; ++t) {
          const int r = b * 32 + t;
          const double wv = W[((size_t)j * fcin + r) * N + n];
          wmax = std::max(wmax, std::fabs(wv));
          w2[r] += wv * wv;
          m2 += m[r] * m[r];
          den += m[r] * m[r] * wv * wv;
        }
        num_w += m2 * wmax * wmax;
      }
  double num_a = 0.0;
  for (int b = 0; b < nb; ++b) {
    double mb = 0.0;
    for (int t = 0; t < 32; ++t) mb = std::max(mb, m[b * 32 + t]);
    for (int t = 0; t < 32; ++t) num_a += mb * mb * w2[b * 32 + t];
  }
  if (!(den > 0.0) || !std::isfinite(num_a + num_w)) return 0.0;     // an all-zero layer: nothing to lose
  return std::hypot(std::sqrt(num_a / den), std::sqrt(num_w / den));
}

int upload_layer(xv_handle* h, Layer& L) {
  const int K = L.K(), N = L.cout;
  // row of the packed weight matrix that holds kernel row k: identity, or tap * cin_pad + channel for a first layer
  // whose frames are padded to whole 32-channel blocks (the padding rows stay zero)
  auto krow = [&](int k) { return L.cin_pad ? (k / L.cin) * L.cin_pad + (k % L.cin) : k; };
  L.Kpad = (int)align_up(L.cin_pad ? L.w * L.cin_pad : K, 32);
  L.Npad = (int)align_up(N, 128);
  const auto& W = T(h, L.kernel_name).data;      // [K][N] (HWIO flattened k-major / [in,out])
  const std::vector<float> no_bias((size_t)N, 0.f);      // resnet convs: use_bias=False (model/resnet.py:31)
  const auto& bias = L.has_bias ? T(h, L.bias_name).data : no_bias;
  std::vector<float> vec((size_t)5 * N, 0.f);
  for (int n = 0; n < N; ++n) { vec[n] = bias[n]; vec[(size_t)4 * N + n] = 1.f; }
  if (L.has_bn) {
    std::vector<double> s, t;
    bn_fold(h, L.bn_scope, N, s, t);
    for (int n = 0; n < N; ++n) {
      vec[(size_t)N + n] = (float)s[n];
      vec[(size_t)2 * N + n] = (float)((double)bias[n] * s[n] + t[n]);
    }
  } else {
    for (int n = 0; n < N; ++n) { vec[(size_t)N + n] = 1.f; vec[(size_t)2 * N + n] = bias[n]; }
  }
  if (!L.alpha_name.empty()) {
    const auto& a = T(h, L.alpha_name).data;
    for (int n = 0; n < N; ++n) vec[(size_t)3 * N + n] = a[n];
  }
  XV_HIP(h, L.vec.alloc(vec.size() * sizeof(float)));
  XV_HIP(h, hipMemcpy(L.vec.p, vec.data(), vec.size() * sizeof(float), hipMemcpyHostToDevice));

  if (L.mode == 4) {                                  // conv0_direct_kernel: the 9 x cout kernel as it is, true BN scale / shift
    std::vector<float> wd((size_t)11 * N);
    for (int k = 0; k < 9; ++k)
      for (int n = 0; n < N; ++n) wd[(size_t)k * N + n] = W[(size_t)k * N + n];
    for (int n = 0; n < N; ++n) { wd[(size_t)9 * N + n] = vec[(size_t)N + n]; wd[(size_t)10 * N + n] = vec[(size_t)2 * N + n]; }
    XV_HIP(h, L.wdir.alloc(wd.size() * sizeof(float)));
    XV_HIP(h, hipMemcpy(L.wdir.p, wd.data(), wd.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  const size_t elems = (size_t)L.Npad * L.Kpad;
  if (!L.use_split) {
    std::vector<float> wt(elems, 0.f);
    for (int k = 0; k < K; ++k)
      for (int n = 0; n < N; ++n) wt[(size_t)n * L.Kpad + k] = W[(size_t)k * N + n];
    XV_HIP(h, L.wt.alloc(elems * sizeof(float)));
    XV_HIP(h, hipMemcpy(L.wt.p, wt.data(), elems * sizeof(float), hipMemcpyHostToDevice));
  } else {
    // split-blocked: row n, block kb: [32 x hi | 32 x lo] for k = 32*kb .. 32*kb+31 (xv_common.h)
    const bool f16 = h->desc.precision == XV_PREC_F16X3 || h->desc.precision == XV_PREC_F16F6;
    float wscale = 1.f;
    if (f16) {
      // fp16 hi/lo keeps 22 significand bits only while the low half stays normal (|w * s| >= 2^-3): scale the layer's
      // weights by a power of two so that the largest lands in [8192, 16384); the epilogue's per-channel scale
      // (and the "ones" vector of the affine-stage endpoints) absorbs 1/s exactly
      float maxabs = 0.f;
      for (size_t i = 0; i < (size_t)K * N; ++i) maxabs = std::max(maxabs, std::fabs(W[i]));
      if (maxabs > 0.f && std::isfinite(maxabs)) {
        int e = 0;
        std::frexp(maxabs, &e);                     // maxabs = m * 2^e, m in [0.5, 1)
        wscale = std::ldexp(1.f, std::min(std::max(14 - e, -24), 24));
      }
    }
    std::vector<uint16_t> sb(elems * 2, 0);
    for (int k = 0; k < K; ++k)
      for (int n = 0; n < N; ++n) {
        const float wv = W[(size_t)k * N + n] * wscale;
        const int kr = krow(k);
        const size_t blk = ((size_t)n * (L.Kpad / 32) + kr / 32) * 64;
        if (f16) {
          const uint16_t a = f32_to_f16_rn(wv);
          sb[blk + (kr & 31)] = a;
          sb[blk + 32 + (kr & 31)] = f32_to_f16_rn(wv - f16_to_f32(a));
        } else {
          const uint16_t a = f32_to_bf16_rn(wv);
          sb[blk + (kr & 31)] = a;
          sb[blk + 32 + (kr & 31)] = f32_to_bf16_rn(wv - bf16_to_f32(a));
        }
      }
    if (wscale != 1.f || L.in_exp != 0) {             // fold 1/s into [bn_scale | ones]; bias / shift are not products
      const float inv = std::ldexp(1.f / wscale, -L.in_exp);          // (and the power of two the input's split copy is kept at)
      for (int n = 0; n < N; ++n) { vec[(size_t)N + n] *= inv; vec[(size_t)4 * N + n] *= inv; }
      XV_HIP(h, hipMemcpy(L.vec.p, vec.data(), vec.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    XV_HIP(h, L.wsb.alloc(elems * 4));
    XV_HIP(h, hipMemcpy(L.wsb.p, sb.data(), elems * 4, hipMemcpyHostToDevice));
    // fragment-major copy for the weights-in-registers kernels (v_mfma_f32_16x16x32 A operand: lane = 16 * k-chunk + row):
    // per (32-channel block, K block) 4 KB = [plane hi/lo][16-channel tile][64 lanes][16 B]; one global_load_dwordx4 of a
    // wave = 1 KB contiguous
    std::vector<uint16_t> fr(elems * 2, 0);
    const size_t nkb = L.Kpad / 32;
    for (size_t n = 0; n < (size_t)L.Npad; ++n)
      for (size_t kb = 0; kb < nkb; ++kb)
        for (int q = 0; q < 8; ++q) {                       // SB chunk q = plane * 4 + k-chunk (8 k values, 16 bytes)
          const int plane = q >> 2, g = q & 3, ct = (int)((n >> 4) & 1);
          const size_t src = (n * nkb + kb) * 64 + (size_t)q * 8;
          const size_t dst = ((((n / 32) * nkb + kb) * 4 + plane * 2 + ct) * 64 + g * 16 + (n & 15)) * 8;
          for (int e = 0; e < 8; ++e) fr[dst + e] = sb[src + e];
        }
    XV_HIP(h, L.wfr.alloc(elems * 4));
    XV_HIP(h, hipMemcpy(L.wfr.p, fr.data(), elems * 4, hipMemcpyHostToDevice));
    if (L.use_f6) {
      // gemm_f6v2_kernel operands (the scaled weights w * wscale, like the f16 halves above):
      //   main  [Npad/32][cin/32][4 NQ tap slots, fw used][2 channel tiles][64 lanes = 16 * k-chunk + channel][8 x f16]      (NQ = ceil(fw / 4))
      //   cross [Npad/32][cin/128][fw macro steps][2 terms: q6(w - f16(w)), q6(f16(w))][2 channel tiles] x { 64 x 16 B codes 0-15 |
      //         64 x 16 B {codes 16-23, scale dword (E8M0 in byte 0), pad} },  lane = 16 * K group + channel
      // (a 3 x 3 grid convolution = three taps along time over the 3 cin contiguous channels of a kernel row: HWIO k-major is
      //  already [kt][kf * cin + c][n])
      const int fw = L.mode == 1 ? 3 : L.w, fcin = L.mode == 1 ? 3 * L.cin : L.cin;
      const int ncb = fcin / 32, NQ = (fw + 3) / 4;
      const size_t main_ct = 64 * 16, cross_ct = 2 * 64 * 16;
      // The cross operands are grouped over QUADS of channel blocks: slot p = fw * (cb & 3) + tap of a quad is K group p & 3 of its macro
      // step p >> 2 -- 4 fw slots = fw macro steps exactly, no zero groups:  [Npad/32][cin/128][fw][2 terms][2 tiles]
      const size_t xsteps = (size_t)(ncb / 4) * fw;
      std::vector<unsigned char> wm((size_t)(L.Npad / 32) * ncb * (4 * NQ) * 2 * main_ct, 0), wx((size_t)(L.Npad / 32) * xsteps * 2 * 2 * cross_ct, 0);
      for (int n = 0; n < L.Npad; ++n) {
        const int nb = n >> 5, ct = (n >> 4) & 1, r16 = n & 15;
        for (int cb = 0; cb < ncb; ++cb)
          for (int j = 0; j < 4 * NQ; ++j) {
            float whi[32], wlo[32];
            uint16_t hh[32];
            for (int t = 0; t < 32; ++t) {
              const float wv = (j < fw && n < N) ? W[((size_t)j * fcin + cb * 32 + t) * N + n] * wscale : 0.f;
              hh[t] = f32_to_f16_rn(wv);
              whi[t] = f16_to_f32(hh[t]);
              wlo[t] = wv - whi[t];
            }
            unsigned char* pm = &wm[((((size_t)nb * ncb + cb) * (4 * NQ) + j) * 2 + ct) * main_ct];
            for (int kc = 0; kc < 4; ++kc) memcpy(pm + (16 * kc + r16) * 16, &hh[8 * kc], 16);
            if (j >= fw) continue;                          // (main weights: tap slots padded to 4 NQ; the cross operands have no padding)
            const int slot = (cb & 3) * fw + j;
            const size_t xstep = (size_t)(cb >> 2) * fw + (slot >> 2);
            const int ln = 16 * (slot & 3) + r16;
            for (int term = 0; term < 2; ++term) {          // term 0 multiplies q6(hi) of the activations, term 1 q6(lo)
              unsigned char* px = &wx[(((((size_t)nb * xsteps + xstep) * 2 + term) * 2) + ct) * cross_ct];
              unsigned char c24[24], sc;
              host_quant32(term == 0 ? wlo : whi, c24, &sc);
              memcpy(px + ln * 16, c24, 16);
              memcpy(px + 1024 + ln * 16, c24 + 16, 8);
              px[1024 + ln * 16 + 8] = sc;
            }
          }
      }
      XV_HIP(h, L.wf6m.alloc(wm.size()));
      XV_HIP(h, hipMemcpy(L.wf6m.p, wm.data(), wm.size(), hipMemcpyHostToDevice));
      XV_HIP(h, L.wf6x.alloc(wx.size()));
      XV_HIP(h, hipMemcpy(L.wf6x.p, wx.data(), wx.size(), hipMemcpyHostToDevice));
    }
  }
  return XV_OK;
}

// Which kernel runs each layer, and in which number format (no device call; ahead of the uploads, which pack the weights for
// that choice): use_split / im2col / cin_pad / use_f6, then the power-of-two exponents of the fp16 split formats.
void choose_kernels(xv_handle* h) {
  for (const Op& op : h->ops) {      // which layers run on the bf16x3 kernel
    if (op.kind != OP_GEMM) continue;
    Layer& L = h->layers[op.layer];
    const Value& vin = h->values[op.in0];
    const bool bf = h->desc.precision != XV_PREC_F32;       // a split format: bf16x3 or f16x3
    if (L.mode == 0) {
      L.im2col = bf && op.in0 == 0;
      L.cin_pad = (L.im2col && L.w <= 9) ? (int)align_up(L.cin, 32) : 0;
      L.use_split = L.im2col || (bf && vin.frame_level && (L.w == 1 || (L.cin % 32 == 0 && L.w <= 9)));   // slab halo of the split kernel
      // two-unit split: the 5-, 7- and 9-tap layers over whole 32-channel blocks (the first layer, K = 5 x 30, stays on the f16 kernel and writes
      // the block format of its reader: gemm_bf16x3_w14p2_kernel<1, 3, true>)
      // (dense layers stay on three units: a one-tap two-unit kernel needs four slabs per macro step = one workgroup per CU, and
      //  with nothing to overlap its prologue and epilogue it was no faster -- profiles/r03/ab_dense_two_unit.txt)
      L.use_f6 = h->desc.precision == XV_PREC_F16F6 && L.use_split && !L.im2col && (L.w == 5 || L.w == 7 || L.w == 9) &&
                 L.cin % 128 == 0 && L.cout % 4 == 0;      // (the kernel takes channel blocks in quads)
    } else {      // grid convolutions: whole SB blocks per tap; conv0 goes through its own im2col
      L.use_split = bf && (L.mode == 4 || L.cin % 32 == 0);
      // two-unit split of the stride-1 3 x 3 convolutions: three taps along time over the 3 C channels of a kernel row
      // (gemm_f6v2_kernel<3, ...>); whole 128-channel tiles only (stage 1 of the default net, 64 channels, is HBM-bound anyway)
      L.use_f6 = h->desc.precision == XV_PREC_F16F6 && h->opt_grid_f6 && L.mode == 1 && L.use_split && L.sw == 1 && L.st == 1 &&
                 L.cin % 128 == 0 && L.cout % 128 == 0;      // (3 cin / 32 channel blocks, taken in quads)
    }
    // a layer whose 32-channel blocks hold magnitudes too far apart for the block-scaled cross terms stays on three units
    if (L.use_f6 && f6_block_spread(h, op, L) > kF6MaxSpread) L.use_f6 = false;
  }
  if (h->desc.precision == XV_PREC_F16X3 || h->desc.precision == XV_PREC_F16F6) {
    for (const Op& op : h->ops) {      // creation order is topological: a value's exponent is known before its readers
      if (op.kind == OP_GEMM) {
        Layer& L = h->layers[op.layer];
        L.in_exp = (L.use_split && !L.im2col && L.mode != 4 && op.in0 > 0) ? h->values[op.in0].sb_exp : 0;
        L.out_exp = act_exponent(h, L);
        h->values[op.out].sb_exp = L.out_exp;
      } else if (op.kind == OP_GRID_MAXPOOL) {
        h->values[op.out].sb_exp = h->values[op.in0].sb_exp;
      }
    }
  }
}

}  // namespace

extern "C" {

int xv_finalize(xv_handle* h) {
  if (!h) return fail(nullptr, XV_ERR_INVALID, "xv_finalize: null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->finalized) return XV_OK;
  for (const auto& kv : h->tensors)
    if (!kv.second.set) return fail(h, XV_ERR_MISSING_TENSOR, "variable '%s' was never set", kv.first.c_str());
  choose_kernels(h);
  DeviceGuard g(h->device);
  if (!g.ok) return fail(h, XV_ERR_HIP, "cannot select HIP device %d", h->device);
  for (auto& L : h->layers) {
    const int rc = upload_layer(h, L);
    if (rc != XV_OK) return rc;
  }
  if (h->desc.pooling_type == XV_POOL_SELF_ATTENTION) {
    const auto& q = T(h, std::string(h->desc.network_type == XV_NET_ETDNN ? "etdnn/" : "tdnn/") + "attention/query").data;
    XV_HIP(h, h->query.alloc(q.size() * sizeof(float)));
    XV_HIP(h, hipMemcpy(h->query.p, q.data(), q.size() * sizeof(float), hipMemcpyHostToDevice));
    {
      const int H = h->desc.att_num_heads, dkh = h->att_dk_h;
      h->key_npad = (int)align_up(h->att_dk, 128);
      std::vector<float> qe((size_t)H * h->key_npad, 0.f);
      for (int hd = 0; hd < H; ++hd)
        for (int d = 0; d < dkh; ++d) {
          const int n = h->desc.att_split_key ? hd * dkh + d : d;
          qe[(size_t)hd * h->key_npad + n] = q[(size_t)hd * dkh + d];
        }
      XV_HIP(h, h->query_eff.alloc(qe.size() * sizeof(float)));
      XV_HIP(h, hipMemcpy(h->query_eff.p, qe.data(), qe.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if (h->desc.att_apply_nonlinear) {
      const int n = h->pool_dim;
      std::vector<double> s, t;
      bn_fold(h, h->post_bn_scope, n, s, t);
      std::vector<float> vec((size_t)3 * n, 0.f);
      for (int i = 0; i < n; ++i) { vec[i] = (float)s[i]; vec[(size_t)n + i] = (float)t[i]; }
      if (!h->post_alpha_name.empty()) {
        const auto& a = T(h, h->post_alpha_name).data;
        for (int i = 0; i < n; ++i) vec[(size_t)2 * n + i] = a[i];
      }
      XV_HIP(h, h->post_vec.alloc(vec.size() * sizeof(float)));
      XV_HIP(h, hipMemcpy(h->post_vec.p, vec.data(), vec.size() * sizeof(float), hipMemcpyHostToDevice));
    }
  }
  XV_HIP(h, h->ovf_flag.alloc(kFlagBufWords * sizeof(int)));
  XV_HIP(h, hipMemset(h->ovf_flag.p, 0, kFlagBufWords * sizeof(int)));
  XV_HIP(h, hipDeviceSynchronize());
  for (auto& kv : h->tensors) { kv.second.data.clear(); kv.second.data.shrink_to_fit(); }
  h->finalized = true;
  return XV_OK;
}

int xv_check_overflow(xv_handle* h, int reset) {
  if (!h) return fail(nullptr, XV_ERR_INVALID, "xv_check_overflow: null handle");
  if (!h->finalized || !h->ovf_flag.p) return 0;
  DeviceGuard g(h->device);
  std::vector<int32_t> w((size_t)kFlagWords + kFeatMaxSlots);
  XV_HIP(h, hipMemcpy(w.data(), h->ovf_flag.p, w.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  int32_t v[2] = {w[0], w[1]};
  for (int i = 0; i < kFeatMaxSlots; ++i) v[1] = std::max(v[1], w[(size_t)kFlagWords + i]);     // non-negative floats order like ints
  if (w[kUttSmallWord]) v[1] = w[kUttSmallWord];                 // an utterance below 2^-8 (flags_snapshot_kernel does the same)
  if (reset) XV_HIP(h, hipMemset(h->ovf_flag.p, 0, w.size() * sizeof(int32_t)));
  return xv_flags_decode(v);
}

int xv_flags_decode(const int32_t* flags) {
  if (!flags) return XV_ERR_INVALID;
  if (flags[0]) return 1;
  if (flags[1] > 0) {                    // bits of the largest |feature| staged (0: no feature staged, or all zero)
    float mx;
    memcpy(&mx, &flags[1], 4);
    if (mx < 0.00390625f) return 2;      // 2^-8
  }
  return 0;
}

int xv_flags_async(xv_handle* h, int32_t* host_flags, void* stream) {
  if (!h || !host_flags) return fail(h, XV_ERR_INVALID, "xv_flags_async: null argument");
  if (!h->finalized || !h->ovf_flag.p) { host_flags[0] = host_flags[1] = 0; return XV_OK; }
  DeviceGuard g(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // pinned (device-accessible) host memory: one small kernel writes the words there and clears them; anything else: a copy + a memset
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, host_flags) == hipSuccess && attr.type == hipMemoryTypeHost) {
    XV_HIP(h, launch_flags_snapshot(static_cast<int*>(h->ovf_flag.p), host_flags, s));
    return XV_OK;
  }
  (void)hipGetLastError();               // (an unregistered pointer makes the query fail: not an error of ours)
  // pageable destination: the words are reduced into device word 1 first, then copied
  XV_HIP(h, launch_flags_snapshot(static_cast<int*>(h->ovf_flag.p), static_cast<int*>(h->ovf_flag.p) + 2, s));
  XV_HIP(h, hipMemcpyAsync(host_flags, static_cast<int*>(h->ovf_flag.p) + 2, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  return XV_OK;
}

}  // extern "C"
