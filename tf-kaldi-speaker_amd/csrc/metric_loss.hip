// Metric-learning loss heads for validation (include/xvec_hip.h, xv_metric_loss): the semi-hard triplet loss
// (model/loss.py:387-527), the angular triplet loss (:530-663, "all" and "hard") and the generalized end-to-end loss
// (:666-734, softmax and contrastive), evaluated per group (a batch) of rows.  The rules are stated in the header and
// restated in numpy by tests/helpers/ref_metric_loss.py; the reference's own float64 twins (model/test_utils.py) pin them
// through tests/golden/metric_*.npz.  Everything is double, from float32 rows.
//
// G(a, b).  Every product of two rows is a chain of v_mfma_f64_16x16x4_f64 (as csrc/backend.hip; operand / result lane layout
// as pinned there): a lane holds, for 16 columns at a time, the four values t = 16 n + 4 (lane >> 4) + m, m = 0 .. 3, of its
// row (lane & 15), and instruction m of the block consumes value m of every lane, so the block adds its 16 products in one
// fixed order and the blocks follow in column order: entry (i, j) is a function of the VALUES of rows i and j alone, whatever
// their position, tile or group (columns past d are zeros and add nothing; rows past the group are zeros and never stored).
// The squared norms n_i are the diagonal of the same chain run on 16 rows against themselves (row_stats_kernel), so
// n_i == G(v_i, v_i) bit for bit: two identical rows are at distance 0 exactly, and a negative that is a bitwise copy of a
// positive has the positive's distance.  tests/test_gpu_metric_loss.py holds the hardware to that (ties, zeros, a group alone
// and in a batch).  G(u_i, e_i) of the ge2e kinds, one value per row, is a lane-strided chain and an xor butterfly instead.
//
// Error.  With unit operands |fl G - G| <= d 2^-53 sum |a_t b_t| <= d 2^-53 whatever the order of the additions, and the
// operands u = x * s carry two more roundings each (s, the product): (d + 8) 2^-53 covers the product, its operands and the few
// operations of a head behind it.  A head multiplies that by its slope: 1, 4, 16 for asoftmax m = 1, 2, 4 (|d pos / dc|), 1 for
// amsoftmax, cos m + sin m |c| / sqrt(1 - c^2) for arcsoftmax, 1 / (2 d) for the square root at distance d (D2 itself carries
// 4 products), 2 |w| for ge2e (the row and its log-sum-exp move by |w| each).  tests/helpers/ref_metric_loss.bounds().
//
// Launches (no workgroup waits for another, no atomics of any kind):
//   1. row_stats_kernel, one wave per 16 rows: s_i = 1 / sqrt(max(G(x_i, x_i), 1e-12)) (1 without `normalize`) and
//      n_i = G(v_i, v_i), v = x s.
//   2. triplet kinds, panel_kernel: a workgroup of 8 waves takes 16-anchor panels of one group (blockIdx.x, + gridDim.x, ...).
//      The panel G(v_i, v_j), 16 x B doubles, lives in LDS while B <= 1024 (128 KiB of the CU's 160) and in a slot of the
//      workspace above.  A wave takes 16-column tiles, four at a time against one load of the anchors; the operands go from
//      global memory straight into the MFMA layout (16 rows x 64 contiguous bytes per load, float4 when the rows are 16-byte
//      aligned), the next 16 columns in flight under the MFMAs of the current ones.  The panel is turned into distances /
//      clipped cosines in place, then mined: the 32 threads of a half-wave share one anchor, find its positives 32 rows at a
//      time with a ballot and scan the negatives of every positive together (k = q, q + 32, ...; min / sum over the half-wave
//      by an xor butterfly); the terms of an anchor are added in row order of the positives.  Trip counts come from B
//      alone (nothing is unrolled on an assumed rows-per-speaker).
//      ge2e kinds, ge2e_kernel: a workgroup takes whole groups and owns a slot ([B, d] class sums, [B, C] similarities).
//      Classes in order of first appearance, a stable counting sort of the rows by class, the class sums in row order (one
//      thread per column), the similarities as 16 x 16 MFMA tiles, then one wave per row: e_i, its own similarity and an online
//      max-shifted log-sum-exp (softmax) or the sigmoids (contrastive) over the row.
//   3. finalize_kernel: one thread per group adds the rows in row order (np.cumsum(rows)[-1]) and normalises.
// The workspace decides only how many slots run at a time: the bits do not depend on it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

#include "wave_reduce.h"
#include "xv_kernels.h"
#include "metric_panel.h"

namespace xv {
namespace {

__global__ __launch_bounds__(kThreads) void panel_kernel(MetricArgs g) {
  extern __shared__ double dyn[];                      // labels [max_rows] (int32), then the panel [16, ldp]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  int32_t* lab = reinterpret_cast<int32_t*>(dyn);
  const int lab_doubles = (g.max_rows + 1) / 2;
  const int d = g.d;
  const double inf = __builtin_inf();

  for (int64_t p = blockIdx.x; p < g.num_panels; p += gridDim.x) {
    __syncthreads();
    const int64_t grp = g.panels[2 * p];
    const int i0 = g.panels[2 * p + 1];
    const int64_t row0 = g.offsets[grp];
    const int B = (int)(g.offsets[grp + 1] - row0);
    const int ldp = B | 1;                             // odd: the anchors of a wave read different banks
    double* pan = g.use_lds ? dyn + lab_doubles : g.slots + (int64_t)blockIdx.x * g.slot_doubles;
    for (int j = tid; j < B; j += kThreads) lab[j] = g.labels[row0 + j];

    // ---- the panel G(v_i, v_j): wave w takes the 16-column tiles tb + w, tb + w + 8, ... four at a time
    {
      const bool a_ok = i0 + lr < B;
      const float* a_row = g.x + (row0 + (a_ok ? i0 + lr : 0)) * g.ldx;
      const double sa = a_ok ? g.scale[row0 + i0 + lr] : 0.0;
      const int ntile = (B + 15) >> 4;
      for (int tb = wave; tb < ntile; tb += kWaves * kNT) {
        const float* b_row[kNT];
        bool b_ok[kNT];
        double sb[kNT];
        d4 acc[kNT];
        int nv = 0;
#pragma unroll
        for (int t = 0; t < kNT; ++t) {
          const int tile = tb + t * kWaves;
          if (tile < ntile) nv = t + 1;
          const int j = tile * 16 + lr;
          b_ok[t] = tile < ntile && j < B;
          b_row[t] = g.x + (row0 + (b_ok[t] ? j : 0)) * g.ldx;
          sb[t] = b_ok[t] ? g.scale[row0 + j] : 0.0;
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[t][e] = 0.0;
        }
        tile_products<float>(a_row, a_ok, sa, g.vec, b_row, b_ok, sb, g.vec, nv, d, acc);
#pragma unroll
        for (int t = 0; t < kNT; ++t) {
          const int j = (tb + t * kWaves) * 16 + lr;
          if (t < nv && j < B) {
#pragma unroll
            for (int e = 0; e < 4; ++e) pan[(lq + 4 * e) * ldp + j] = acc[t][e];
          }
        }
      }
    }
    __syncthreads();

    // ---- distances / clipped cosines in place
    for (int idx = tid; idx < kPanelAnchors * B; idx += kThreads) {
      const int a = idx / B, j = idx - a * B;
      const int i = i0 + a;
      if (i >= B) break;
      const double gij = pan[a * ldp + j];
      double v;
      if (g.kind == XV_METRIC_SEMIHARD) {
        const double d2 = fmax(g.nrm[row0 + i] - 2.0 * gij + g.nrm[row0 + j], 0.0);
        v = i == j ? 0.0 : (g.squared ? d2 : sqrt(d2));
      } else {
        v = fmin(fmax(gij, -1.0), 1.0);
      }
      pan[a * ldp + j] = v;
    }
    __syncthreads();

    // ---- mining: the 32 threads of a half-wave share one anchor.  Every trip count below is the same in the 32 threads, so
    // the xor shuffles (distance < 32) only ever read lanes that run the same instruction.
    const int a = tid / kQ, q = tid % kQ;
    const int i = i0 + a;
    if (i < B) {
      const double* row = pan + a * ldp;
      const int li = lab[i];
      double mx = -inf;                    // over the negatives: the largest distance / cosine
      int nneg = 0;
#pragma unroll 4
      for (int k = q; k < B; k += kQ)
        if (lab[k] != li) {
          mx = fmax(mx, row[k]);
          ++nneg;
        }
      mx = half_max(mx);
      nneg = half_sum(nneg);
      double sum = 0.0;
      long long cnt = 0, aux = 0;
      if (g.kind == XV_METRIC_ANGULAR_HARD) {
        double hp = inf;                   // hardest positive, the anchor itself included
        for (int j = q; j < B; j += kQ)
          if (lab[j] == li) hp = fmin(hp, pos_value(row[j], g));
        hp = half_min(hp);
        sum = nneg ? fmax(mx - hp, 0.0) : 0.0;
        cnt = 1;
      } else if (nneg) {
        for (int j0 = 0; j0 < B; j0 += kQ) {
          // the positives among the rows j0 .. j0 + 31, in row order
          const int jq = j0 + q;
          const bool is_pos = jq < B && jq != i && lab[jq] == li;
          unsigned todo = (unsigned)(__ballot(is_pos) >> (32 * ((tid & 63) >> 5)));
          while (todo) {
            const int j = j0 + __builtin_ctz(todo);
            todo &= todo - 1;
            if (g.kind == XV_METRIC_SEMIHARD) {
              const double dij = row[j];
              double mn = inf;
#pragma unroll 4
              for (int k = q; k < B; k += kQ) {
                const double dk = row[k];
                if (lab[k] != li && dk > dij && dk < mn) mn = dk;
              }
              mn = half_min(mn);
              const double z = mn < inf ? mn : mx;
              sum += fmax(g.margin + dij - z, 0.0);
              ++cnt;
            } else {
              const double pj = pos_value(row[j], g);
              double ps = 0.0;
              int pc = 0;
#pragma unroll 4
              for (int k = q; k < B; k += kQ)
                if (lab[k] != li) {
                  const double t = row[k] - pj;
                  ps += fmax(t, 0.0);
                  pc += t > kEps;
                }
              sum += half_sum(ps);
              cnt += half_sum(pc);
              aux += nneg;
            }
          }
        }
      }
      if (q == 0) {
        g.row_loss[row0 + i] = sum;
        g.row_count[row0 + i] = cnt;
        g.aux[row0 + i] = aux;
      }
    }
  }
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

__device__ __forceinline__ double sigmoid(double z) {
  const double e = exp(-fabs(z));
  return z >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}

__global__ __launch_bounds__(kThreads) void ge2e_kernel(MetricArgs g) {
  __shared__ uint16_t cls[kMaxRows];          // class of a row
  __shared__ uint16_t perm[kMaxRows];         // rows sorted by class, row order inside a class
  __shared__ uint16_t start[kMaxRows + 1];    // class -> its range of perm
  __shared__ double cscale[kMaxRows];         // 1 / |class sum|
  __shared__ int s_classes;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int d = g.d;
  const double inf = __builtin_inf();
  double* csum = g.slots + (int64_t)blockIdx.x * g.slot_doubles;      // [classes, d]
  double* sim = csum + (int64_t)g.max_rows * d;                       // [B, classes]

  for (int64_t grp = blockIdx.x; grp < g.num_groups; grp += gridDim.x) {
    __syncthreads();
    const int64_t row0 = g.offsets[grp];
    const int B = (int)(g.offsets[grp + 1] - row0);
    const int32_t* lab = g.labels + row0;
    const float* x = g.x + row0 * g.ldx;
    const double* sc = g.scale + row0;

    // ---- classes in order of first appearance; rows sorted by class
    for (int j = tid; j < B; j += kThreads) {
      const int32_t l = lab[j];
      int f = 0;
      while (lab[f] != l) ++f;            // ends at f == j at the latest
      cls[j] = (uint16_t)f;
    }
    __syncthreads();
    if (tid == 0) {
      int n = 0;
      for (int j = 0; j < B; ++j) {
        const int f = cls[j];
        if (f == j) {
          start[n] = 0;
          cls[j] = (uint16_t)n++;
        } else {
          cls[j] = cls[f];
        }
      }
      for (int j = 0; j < B; ++j) ++start[cls[j]];
      int pos = 0;
      for (int c = 0; c < n; ++c) {       // counts -> first free position
        const int cnt = start[c];
        start[c] = (uint16_t)pos;
        pos += cnt;
      }
      for (int j = 0; j < B; ++j) perm[start[cls[j]]++] = (uint16_t)j;
      for (int c = n; c > 0; --c) start[c] = start[c - 1];      // ends -> begins
      start[0] = 0;
      s_classes = n;
    }
    __syncthreads();
    const int C = s_classes;

    // ---- class sums in row order, one thread per column
    for (int t = tid; t < d; t += kThreads)
      for (int c = 0; c < C; ++c) {
        double acc = 0.0;
        for (int k = start[c]; k < start[c + 1]; ++k) {
          const int j = perm[k];
          acc += (double)x[(int64_t)j * g.ldx + t] * sc[j];
        }
        csum[(int64_t)c * d + t] = acc;
      }
    __syncthreads();
    for (int c = wave; c < C; c += kWaves) {
      double pp = 0.0;
      for (int t = lane; t < d; t += 64) {
        const double v = csum[(int64_t)c * d + t];
        pp = fma(v, v, pp);
      }
      pp = wave_sum_f64(pp);
      if (lane == 0) cscale[c] = 1.0 / sqrt(fmax(pp, kEps));
    }
    __syncthreads();

    // ---- sim(i, c) = G(u_i, chat_c): a wave takes 16-row tiles against the class tiles, four at a time
    {
      const int nrt = (B + 15) >> 4, nct = (C + 15) >> 4;
      for (int rt = wave; rt < nrt; rt += kWaves) {
        const bool a_ok = rt * 16 + lr < B;
        const float* a_row = x + (int64_t)(a_ok ? rt * 16 + lr : 0) * g.ldx;
        const double sa = a_ok ? sc[rt * 16 + lr] : 0.0;
        for (int cb = 0; cb < nct; cb += kNT) {
          const double* b_row[kNT];
          bool b_ok[kNT];
          double sb[kNT];
          d4 acc[kNT];
          const int nv = nct - cb < kNT ? nct - cb : kNT;
#pragma unroll
          for (int t = 0; t < kNT; ++t) {
            const int c = (cb + t) * 16 + lr;
            b_ok[t] = c < C;
            b_row[t] = csum + (int64_t)(b_ok[t] ? c : 0) * d;
            sb[t] = b_ok[t] ? cscale[c] : 0.0;
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[t][e] = 0.0;
          }
          tile_products<double>(a_row, a_ok, sa, g.vec, b_row, b_ok, sb, false, nv, d, acc);
#pragma unroll
          for (int t = 0; t < kNT; ++t) {
            const int c = (cb + t) * 16 + lr;
            if (t < nv && c < C) {
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const int i = rt * 16 + lq + 4 * e;
                if (i < B) sim[(int64_t)i * C + c] = acc[t][e];
              }
            }
          }
        }
      }
    }
    __syncthreads();

    // ---- one wave per row
    for (int i = wave; i < B; i += kWaves) {
      const int c0 = cls[i];
      const float* xi = x + (int64_t)i * g.ldx;
      const double si = sc[i];
      const double* own = csum + (int64_t)c0 * d;
      double pp = 0.0;
      for (int t = lane; t < d; t += 64) {
        const double wv = own[t] - (double)xi[t] * si;
        pp = fma(wv, wv, pp);
      }
      const double es = 1.0 / sqrt(fmax(wave_sum_f64(pp), kEps));
      pp = 0.0;
      for (int t = lane; t < d; t += 64) {
        const double u = (double)xi[t] * si;
        pp = fma(u, (own[t] - u) * es, pp);
      }
      const double z_own = g.w * wave_sum_f64(pp) + g.b;

      // lane c & 63 keeps the running state of class c
      double lm = -inf, ls = 0.0;          // online log-sum-exp
      double best = -inf, sig = 0.0;       // arg-max of z; largest sigmoid of another class
      int best_c = kMaxRows;
      for (int c = lane; c < C; c += 64) {
        const double z = c == c0 ? z_own : g.w * sim[(int64_t)i * C + c] + g.b;
        if (z > lm) {
          ls = ls * exp(lm - z) + 1.0;
          lm = z;
        } else {
          ls += exp(z - lm);
        }
        if (z > best) {
          best = z;
          best_c = c;
        }
        if (c != c0) sig = fmax(sig, sigmoid(z));
      }
      const double m = wave_max(lm);
      const double total = wave_sum_f64(lm > -inf ? ls * exp(lm - m) : 0.0);
      const double top = wave_max(best);
      int cand = best == top ? best_c : kMaxRows;       // the earliest class among equals
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o));
      const double smax = wave_max(sig);
      if (lane == 0) {
        if (cand >= C) cand = c0;                        // NaN similarities: no class compares greater
        const int32_t top1 = lab[perm[start[cand]]];
        const double out = g.kind == XV_METRIC_GE2E_SOFTMAX ? (m + log(total)) - z_own : 1.0 - sigmoid(z_own) + smax;
        g.row_loss[row0 + i] = out;
        g.row_count[row0 + i] = 1;
        g.aux[row0 + i] = top1 == lab[i];
        if (g.row_top1) g.row_top1[row0 + i] = top1;
      }
    }
  }
}

struct Layout {
  int64_t panels, max_rows, rows;
  int64_t off_panels, off_scale, off_nrm, off_aux, off_slots, slot_bytes;
};

// offsets: checked by the caller (ascending, 1 .. 4096 rows per group)
Layout layout(int64_t num_groups, const int64_t* offsets, int d, int kind) {
  Layout l = {};
  for (int64_t g = 0; g < num_groups; ++g) {
    const int64_t b = offsets[g + 1] - offsets[g];
    l.max_rows = std::max(l.max_rows, b);
    l.panels += (b + kPanelAnchors - 1) / kPanelAnchors;
  }
  l.rows = offsets[num_groups];
  const bool ge2e = kind == XV_METRIC_GE2E_SOFTMAX || kind == XV_METRIC_GE2E_CONTRASTIVE;
  if (ge2e) l.panels = 0;
  l.off_panels = round256(8 * (num_groups + 1));
  l.off_scale = l.off_panels + round256(8 * l.panels);
  l.off_nrm = l.off_scale + round256(8 * l.rows);
  l.off_aux = l.off_nrm + round256(8 * l.rows);
  l.off_slots = l.off_aux + round256(8 * l.rows);
  if (ge2e)
    l.slot_bytes = round256(8 * l.max_rows * ((int64_t)d + l.max_rows));      // class sums [B, d], similarities [B, B]
  else
    l.slot_bytes = l.max_rows > kPanelLdsRows ? round256(8 * kPanelAnchors * (l.max_rows | 1)) : 0;
  return l;
}

void free_table(void* p) { delete static_cast<std::vector<int64_t>*>(p); }

}  // namespace

int64_t metric_loss_slot_bytes(int max_rows, int d, int kind) {
  const int64_t offsets[2] = {0, max_rows};
  return layout(1, offsets, d, kind).slot_bytes;
}

int64_t metric_loss_workspace_bytes(int64_t num_groups, const int64_t* offsets, int d, int kind) {
  const Layout l = layout(num_groups, offsets, d, kind);
  return l.off_slots + l.slot_bytes;
}

hipError_t launch_metric_loss(const float* x, int64_t ldx, const int64_t* offsets, int64_t num_groups, int d, const int32_t* labels,
                              int kind, int pos_head, double margin, int squared, int normalize, double w, double b,
                              double* row_loss, int64_t* row_count, int32_t* row_top1, double* group_loss, int64_t* group_count,
                              void* ws, int64_t ws_bytes, hipStream_t stream) {
  const Layout l = layout(num_groups, offsets, d, kind);
  const bool ge2e = l.panels == 0;
  char* base = static_cast<char*>(ws);

  // the group and panel tables, one copy; freed in stream order behind it
  auto* table = new std::vector<int64_t>((size_t)(l.off_scale / 8), 0);
  std::copy(offsets, offsets + num_groups + 1, table->begin());
  if (!ge2e) {
    int32_t* pt = reinterpret_cast<int32_t*>(table->data() + l.off_panels / 8);
    for (int64_t g = 0; g < num_groups; ++g)
      for (int64_t a = 0; a < offsets[g + 1] - offsets[g]; a += kPanelAnchors) {
        *pt++ = (int32_t)g;
        *pt++ = (int32_t)a;
      }
  }
  hipError_t e = hipMemcpyAsync(ws, table->data(), (size_t)l.off_scale, hipMemcpyHostToDevice, stream);

  MetricArgs a = {};
  a.x = x;
  a.ldx = ldx;
  a.d = d;
  a.num_groups = num_groups;
  a.offsets = reinterpret_cast<const int64_t*>(base);
  a.panels = reinterpret_cast<const int32_t*>(base + l.off_panels);
  a.num_panels = l.panels;
  a.labels = labels;
  a.scale = reinterpret_cast<double*>(base + l.off_scale);
  a.nrm = reinterpret_cast<double*>(base + l.off_nrm);
  a.aux = reinterpret_cast<int64_t*>(base + l.off_aux);
  a.kind = kind;
  a.head = pos_head;
  a.m = pos_head == XV_LOSS_ASOFTMAX ? (int)margin : 0;
  a.squared = squared;
  a.normalize = kind == XV_METRIC_SEMIHARD ? normalize : 1;
  a.need_nrm = kind == XV_METRIC_SEMIHARD;
  a.margin = margin;
  a.cosm = std::cos(margin);
  a.sinm = std::sin(margin);
  a.thr = std::cos(M_PI - margin);
  a.w = w;
  a.b = b;
  a.row_loss = row_loss;
  a.row_count = row_count;
  a.row_top1 = row_top1;
  a.group_loss = group_loss;
  a.group_count = group_count;
  a.slots = reinterpret_cast<double*>(base + l.off_slots);
  a.slot_doubles = l.slot_bytes / 8;
  a.use_lds = l.max_rows <= kPanelLdsRows;
  a.max_rows = (int)l.max_rows;
  a.vec = (ldx & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;

  if (e == hipSuccess) {
    const int64_t r0 = offsets[0], r1 = offsets[num_groups];
    hipLaunchKernelGGL(row_stats_kernel, dim3((unsigned)((r1 - r0 + 63) / 64)), dim3(256), 0, stream, a, r0, r1);
    e = hipGetLastError();
  }
  int64_t slots = l.slot_bytes ? std::min<int64_t>((ws_bytes - l.off_slots) / l.slot_bytes, kMaxSlots) : 0;
  if (e == hipSuccess && ge2e) {
    hipLaunchKernelGGL(ge2e_kernel, dim3((unsigned)std::max<int64_t>(std::min(slots, num_groups), 1)), dim3(kThreads), 0, stream, a);
    e = hipGetLastError();
  } else if (e == hipSuccess) {
    const size_t panel_bytes = (size_t)kPanelAnchors * (size_t)(l.max_rows | 1) * sizeof(double);
    const size_t lds = (size_t)((l.max_rows + 1) / 2) * sizeof(double) + (a.use_lds ? panel_bytes : 0);
    {
      static std::mutex mu;            // per-device attribute; any thread may make the first launch on a device
      static bool set_for[64] = {};
      int dev = 0;
      if (hipGetDevice(&dev) != hipSuccess) dev = 0;
      std::lock_guard<std::mutex> lock(mu);
      if (!set_for[dev & 63]) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(panel_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(kPanelLdsRows / 2 * sizeof(double) + kPanelAnchors * (kPanelLdsRows | 1) * sizeof(double)));
        if (e == hipSuccess) set_for[dev & 63] = true;
      }
    }
    if (e == hipSuccess) {
      const int64_t grid = a.use_lds ? std::min<int64_t>(l.panels, 1 << 20) : std::max<int64_t>(std::min(slots, l.panels), 1);
      hipLaunchKernelGGL(panel_kernel, dim3((unsigned)grid), dim3(kThreads), lds, stream, a);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)((num_groups + 63) / 64)), dim3(64), 0, stream, a);
    e = hipGetLastError();
  }
  if (hipLaunchHostFunc(stream, free_table, table) != hipSuccess) {
    (void)hipStreamSynchronize(stream);
    delete table;
  }
  return e;
}

}  // namespace xv
