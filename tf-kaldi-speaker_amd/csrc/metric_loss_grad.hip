// Gradients of the triplet heads (include/xvec_hip.h, xv_metric_loss_grad): the semi-hard triplet loss and the angular triplet
// loss ("all", "hard") with their forward outputs, per group of rows.  The forward is that of csrc/metric_loss.hip: the product
// chain, the row statistics, the mining order and the group sums come from csrc/metric_panel.h, so row_loss, row_count,
// group_loss and group_count are the bits xv_metric_loss writes.  tests/helpers/ref_metric_grad.py restates the rule below in
// numpy float64 and tests/test_metric_grad_host.py holds that to torch.autograd.
//
// The rule.  L_g is the group loss; comparisons, masks, counts and the normalisers are constants.
//   Hinge: max(t, 0) passes 1 iff t > 0.  The clamp of D2 is a hinge too: it passes iff n_i - 2 G + n_j > 0, i.e. D2 > 0.
//   Selections (the semi-hard negative, hp_i and hn_i of HARD) send their gradient to ONE element, the lowest column among
//   equals (TensorFlow splits a tie evenly: parity unpinned on exact ties only).
//   SEMIHARD: an active pair (i, j) adds +1 at d(i, j) and -1 at d(i, k*); dd/dD2 = 1 (`squared`), else 1 / (2 d) where D2 > 0
//     and 0 where D2 == 0 (the reference's mask * 1e-16, model/common.py:86-92: duplicate rows give 0, never inf);
//     D2 = n_i - 2 G(v_i, v_j) + n_j with n_i = G(v_i, v_i) differentiated: dD2/dv_i = 2 (v_i - v_j).
//   ALL: every triplet with t > 0 adds +1 at c(i, k) and -pos'(c(i, j)) at c(i, j).
//   HARD: a row with a negative and hn_i - hp_i > 0 adds +1 / B at c(i, k*) and -pos'(c(i, j*)) / B at c(i, j*); j* == i carries
//     nothing (c(i, i) is the constant 1; TensorFlow would form inf * 0 there for arcsoftmax).
//   pos': asoftmax 1 (m = 1), 4 |c| (m = 2), s3 (32 c^3 - 16 c) (m = 4), the signs being constants; amsoftmax 1; arcsoftmax
//     cos m + c sin m / sqrt(1 - c^2), negated on the branch c <= cos(pi - m).
//   Clip: dc/dG = 1 for -1 < G < 1, else 0, so pos' is never evaluated at |c| = 1.
//   Normalisation (`normalize`, always for the angular kinds): gx_i = s_i (gu_i - (gu_i . u_i) u_i) where sum x^2 > 1e-12, else
//     s_i gu_i (the max branch is a constant).  The test is s_i < 1e6, s_i being the forward's 1 / sqrt(max(sum x^2, 1e-12)).
//   grad_x[i] = float32(grad_scale dL_g / dx_i): everything before is double.
//
// Launches (no workgroup waits for another, no atomics of any kind, every trip count a function of B and d alone):
//   1. row_stats_kernel (metric_panel.h): s_i and n_i.
//   then, for as many groups at a time as the workspace has slots (a slot: W [B, B] and HV [B, d] doubles):
//   2. grad_panel_kernel: a workgroup of 4 waves takes 8-anchor panels of one group.  The panel G(v_i, v_j) (8 x B doubles) and the
//      coefficient counts (8 x B int32) live in LDS: 100 KiB at B = 1024, which is why the panel has 8 anchors and not the
//      forward's 16 (the upper half of the MFMA's 16 rows is fed zeros; an entry is a function of its two rows alone, so the bits
//      are the forward's).  The mining is the forward's, half-wave per anchor, with (value, column) minima for the selections.
//      The coefficients are small integers per (anchor, column): 1 for an active positive and the number of positives that
//      selected a negative (SEMIHARD), the number of active negatives of a positive and of active positives of a negative
//      (ALL), two ones (HARD).  Lane q of the half-wave is the only one that touches the columns k = q mod 32 of its anchor's
//      counts, so they need neither atomics nor barriers.  The half-wave then writes row i of W = dL / dM before normalisation
//      (M = D2 resp. the clipped cosine): the count times the derivative factor, every entry of the row, zeros included.
//   3. hv_kernel: HV = (W + W^T) V as v_mfma_f64_16x16x4_f64 tiles, one wave per 16 x 16 tile, the blocks of 16 rows k in order.
//      The transpose term is why W goes through memory: a panel does not see the other anchors' rows.
//   4. grad_rows_kernel, one wave per row: SEMIHARD gv_i = 2 (rowsum(H)_i v_i - HV_i), cosine kinds gv_i = HV_i; the
//      normalisation backward; the group's normaliser from its row counts (integers: exact in any order); one rounding to float32.
//   5. finalize_kernel (metric_panel.h): the group sums.
// Every sum is taken in an order fixed by (B, d), every buffer entry that is read was written by this call, and the slot a group
// gets decides nothing: a group's outputs are the same bits alone or in a batch, for every workspace and whatever it held.
//
// Error of an element g = grad_x[i, t].  With kappa = grad_scale / normaliser, H = W + W^T and a_it = |kappa| s_i sum_k
// |H_ik| (|v_it| + |v_kt|) (SEMIHARD, doubled) resp. |kappa| s_i sum_k |H_ik| |u_kt| the absolute sum of the element's terms:
//   - the final rounding, 2^-24 |g|;
//   - the sums: every product and addition is one double rounding, a chain of B terms, then d terms for the projection:
//     (B + d + 32) 2^-53 (a_it + |u_it| sum_t' a_it' |u_it'|);
//   - the derivative factors, evaluated on a computed c or D2 that is within unit = (d + 8) 2^-53 (4 unit max(n) for D2) of the
//     exact one: |delta W_ik| <= count |pos''(c)| unit resp. count unit max(n) / d^3 (|d(1 / (2 d)) / dD2| = 1 / (4 d^3)), carried
//     through the same sums.  pos'' = 0 (m = 1, amsoftmax), 4 (m = 2), |96 c^2 - 16| (m = 4), sin m / (1 - c^2)^(3/2) (arcsoftmax).
// tests/helpers/ref_metric_grad.bounds() states this bar; decisions (which terms are active, which element is selected) are
// held apart by the margins the tests assert.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <mutex>
#include <vector>

#include "metric_panel.h"

namespace xv {
namespace {

constexpr int kGThreads = 256;
constexpr int kGWaves = kGThreads / 64;
constexpr int kGAnchors = kGThreads / kQ;        // a half-wave per anchor, as in the forward
static_assert(kGAnchors == 8, "8-anchor panels: panel and counts of a 1024-row group fit the LDS");
constexpr int kGradMaxRows = 1024;
constexpr int kGradMaxSlots = 64;

struct GradArgs {
  MetricArgs m;            // m.panels: the 8-anchor panels of every group, group by group
  int64_t g0;              // the first group of this round: group g works in slot g - g0
  int64_t p0, p1;          // the panels of the round's groups
  int ngroups;             // groups of the round
  double* slots;           // per slot: W [max_rows, max_rows], HV [max_rows, d]
  int64_t slot_doubles;
  float* gx;
  int64_t ldg;
  double grad_scale;
};

// the least value over the half-wave and the lowest column that holds it; the same pair in every lane
__device__ __forceinline__ void half_argmin(double& v, int& c) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const int oc = __shfl_xor(c, o);
    if (ov < v || (ov == v && oc < c)) {
      v = ov;
      c = oc;
    }
  }
}

__device__ __forceinline__ void half_argmax(double& v, int& c) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const int oc = __shfl_xor(c, o);
    if (ov > v || (ov == v && oc < c)) {
      v = ov;
      c = oc;
    }
  }
}

// d pos / dc for -1 < c < 1 (the signs of pos_value are constants)
__device__ __forceinline__ double pos_slope(double c, const MetricArgs& g) {
  if (g.head == XV_LOSS_ASOFTMAX) {
    if (g.m == 1) return 1.0;
    if (g.m == 2) return 4.0 * fabs(c);
    const double s3 = sgn(2.0 * c * c - 1.0) * sgn(c);
    return s3 * (32.0 * c * c * c - 16.0 * c);
  }
  if (g.head == XV_LOSS_AMSOFTMAX) return 1.0;
  const double dt = g.cosm + c * g.sinm / sqrt(1.0 - c * c);
  return c <= g.thr ? -dt : dt;
}

__global__ __launch_bounds__(kGThreads) void grad_panel_kernel(GradArgs ga) {
  const MetricArgs& g = ga.m;
  extern __shared__ double dyn[];                      // labels [max_rows] (int32), the panel [8, max_rows | 1], the counts [8, max_rows]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  int32_t* lab = reinterpret_cast<int32_t*>(dyn);
  double* pan = dyn + (g.max_rows + 1) / 2;
  int32_t* coef = reinterpret_cast<int32_t*>(pan + kGAnchors * (g.max_rows | 1));
  const int d = g.d;
  const double inf = __builtin_inf();

  for (int64_t p = ga.p0 + blockIdx.x; p < ga.p1; p += gridDim.x) {
    __syncthreads();
    const int64_t grp = g.panels[2 * p];
    const int i0 = g.panels[2 * p + 1];
    const int64_t row0 = g.offsets[grp];
    const int B = (int)(g.offsets[grp + 1] - row0);
    const int ldp = B | 1;
    double* W = ga.slots + (grp - ga.g0) * ga.slot_doubles;
    for (int j = tid; j < B; j += kGThreads) lab[j] = g.labels[row0 + j];
    for (int j = tid; j < kGAnchors * B; j += kGThreads) coef[j] = 0;

    // ---- the panel G(v_i, v_j): the forward's chain; the rows 8 .. 15 of the MFMA's A operand are zeros and never stored
    {
      const bool a_ok = lr < kGAnchors && i0 + lr < B;
      const float* a_row = g.x + (row0 + (a_ok ? i0 + lr : 0)) * g.ldx;
      const double sa = a_ok ? g.scale[row0 + i0 + lr] : 0.0;
      const int ntile = (B + 15) >> 4;
      for (int tb = wave; tb < ntile; tb += kGWaves * kNT) {
        const float* b_row[kNT];
        bool b_ok[kNT];
        double sb[kNT];
        d4 acc[kNT];
        int nv = 0;
#pragma unroll
        for (int t = 0; t < kNT; ++t) {
          const int tile = tb + t * kGWaves;
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
          const int j = (tb + t * kGWaves) * 16 + lr;
          if (t < nv && j < B) {
#pragma unroll
            for (int e = 0; e < kGAnchors / 4; ++e) pan[(lq + 4 * e) * ldp + j] = acc[t][e];
          }
        }
      }
    }
    __syncthreads();

    // ---- distances / clipped cosines in place
    for (int idx = tid; idx < kGAnchors * B; idx += kGThreads) {
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

    // ---- mining, in the forward's order; lane q alone touches the counts of the columns q, q + 32, ... of its anchor
    const int a = tid / kQ, q = tid % kQ;
    const int i = i0 + a;
    if (i < B) {
      const double* row = pan + a * ldp;
      int32_t* cf = coef + a * B;
      const int li = lab[i];
      double mx = -inf;
      int kmx = INT_MAX, nneg = 0;
#pragma unroll 4
      for (int k = q; k < B; k += kQ)
        if (lab[k] != li) {
          if (row[k] > mx) {
            mx = row[k];
            kmx = k;
          }
          ++nneg;
        }
      half_argmax(mx, kmx);
      nneg = half_sum(nneg);
      double sum = 0.0;
      long long cnt = 0, aux = 0;
      if (g.kind == XV_METRIC_ANGULAR_HARD) {
        double hp = inf;
        int jhp = INT_MAX;
        for (int j = q; j < B; j += kQ)
          if (lab[j] == li) {
            const double pv = pos_value(row[j], g);
            if (pv < hp) {
              hp = pv;
              jhp = j;
            }
          }
        half_argmin(hp, jhp);
        sum = nneg ? fmax(mx - hp, 0.0) : 0.0;
        cnt = 1;
        if (nneg && mx - hp > 0.0) {
          if (q == (kmx & (kQ - 1))) cf[kmx] = 1;
          if (jhp != i && jhp < B && q == (jhp & (kQ - 1))) cf[jhp] = 1;
        }
      } else if (nneg) {
        for (int j0 = 0; j0 < B; j0 += kQ) {
          const int jq = j0 + q;
          const bool is_pos = jq < B && jq != i && lab[jq] == li;
          unsigned todo = (unsigned)(__ballot(is_pos) >> (32 * ((tid & 63) >> 5)));
          while (todo) {
            const int j = j0 + __builtin_ctz(todo);
            todo &= todo - 1;
            if (g.kind == XV_METRIC_SEMIHARD) {
              const double dij = row[j];
              double mn = inf;
              int kmn = INT_MAX;
#pragma unroll 4
              for (int k = q; k < B; k += kQ) {
                const double dk = row[k];
                if (lab[k] != li && dk > dij && dk < mn) {
                  mn = dk;
                  kmn = k;
                }
              }
              half_argmin(mn, kmn);
              const double z = mn < inf ? mn : mx;
              const int kz = mn < inf ? kmn : kmx;
              const double term = g.margin + dij - z;
              sum += fmax(term, 0.0);
              ++cnt;
              if (term > 0.0) {
                if (q == (j & (kQ - 1))) cf[j] = 1;
                if (q == (kz & (kQ - 1))) cf[kz] += 1;
              }
            } else {
              const double pj = pos_value(row[j], g);
              double ps = 0.0;
              int pc = 0, pa = 0;
#pragma unroll 4
              for (int k = q; k < B; k += kQ)
                if (lab[k] != li) {
                  const double t = row[k] - pj;
                  ps += fmax(t, 0.0);
                  pc += t > kEps;
                  if (t > 0.0) {
                    ++pa;
                    cf[k] += 1;
                  }
                }
              sum += half_sum(ps);
              cnt += half_sum(pc);
              aux += nneg;
              pa = half_sum(pa);
              if (q == (j & (kQ - 1))) cf[j] = pa;
            }
          }
        }
      }
      if (q == 0) {
        g.row_loss[row0 + i] = sum;
        g.row_count[row0 + i] = cnt;
        g.aux[row0 + i] = aux;
      }

      // ---- row i of W = dL / dM before normalisation: the count times the derivative factor
      double* wrow = W + (int64_t)i * B;
      for (int k = q; k < B; k += kQ) {
        const int n = cf[k];
        const double val = row[k];
        const bool same = lab[k] == li;
        double w = 0.0;
        if (n != 0) {
          if (g.kind == XV_METRIC_SEMIHARD) {
            const double f = val > 0.0 ? (g.squared ? 1.0 : 1.0 / (2.0 * val)) : 0.0;
            w = same ? (double)n * f : -(double)n * f;
          } else if (val > -1.0 && val < 1.0) {
            w = same ? -(double)n * pos_slope(val, g) : (double)n;
          }
        }
        wrow[k] = w;
      }
    }
  }
}

// HV = (W + W^T) V: blockIdx.x = (group of the round, 16-row tile), blockIdx.y = 64 columns, a wave per 16 of them
__global__ __launch_bounds__(kGThreads) void hv_kernel(GradArgs ga) {
  const MetricArgs& g = ga.m;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int tiles = (g.max_rows + 15) >> 4;
  const int64_t grp = ga.g0 + blockIdx.x / tiles;
  const int i0 = (blockIdx.x % tiles) * 16;
  const int64_t row0 = g.offsets[grp];
  const int B = (int)(g.offsets[grp + 1] - row0);
  const int t0 = (blockIdx.y * kGWaves + wave) * 16;
  if (i0 >= B || t0 >= g.d) return;
  const double* W = ga.slots + (grp - ga.g0) * ga.slot_doubles;
  double* HV = ga.slots + (grp - ga.g0) * ga.slot_doubles + (int64_t)g.max_rows * g.max_rows;
  const int i = i0 + lr, t = t0 + lr;
  const bool i_ok = i < B, t_ok = t < g.d;
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < B; k0 += 16) {
    double ha[4], vb[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int k = k0 + 4 * lq + m;
      const bool k_ok = k < B;
      ha[m] = (i_ok && k_ok) ? W[(int64_t)i * B + k] + W[(int64_t)k * B + i] : 0.0;
      vb[m] = (k_ok && t_ok) ? (double)g.x[(row0 + k) * g.ldx + t] * g.scale[row0 + k] : 0.0;
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ha[m], vb[m], acc, 0, 0, 0);
  }
  if (t_ok) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = i0 + lq + 4 * e;
      if (r < B) HV[(int64_t)r * g.d + t] = acc[e];
    }
  }
}

// one wave per row: blockIdx.x = group of the round, blockIdx.y * 4 + wave = row
__global__ __launch_bounds__(kGThreads) void grad_rows_kernel(GradArgs ga) {
  const MetricArgs& g = ga.m;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t grp = ga.g0 + blockIdx.x;
  const int64_t row0 = g.offsets[grp];
  const int B = (int)(g.offsets[grp + 1] - row0);
  const int i = blockIdx.y * kGWaves + wave;
  if (i >= B) return;
  const int d = g.d;
  const double* W = ga.slots + (grp - ga.g0) * ga.slot_doubles;
  const double* hv = W + (int64_t)g.max_rows * g.max_rows + (int64_t)i * d;
  const float* xi = g.x + (row0 + i) * g.ldx;
  const double s = g.scale[row0 + i];

  long long total = 0;                               // the group's count: integers, exact in any order
  for (int r = lane; r < B; r += 64) total += g.row_count[row0 + r];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, 64);
  const double denom = g.kind == XV_METRIC_SEMIHARD ? fmax((double)total, 1e-16)
                       : g.kind == XV_METRIC_ANGULAR_ALL ? (double)total + 1e-16 : (double)B;
  const double kappa = ga.grad_scale / denom;

  double rs = 0.0;
  if (g.kind == XV_METRIC_SEMIHARD) {
    for (int k = lane; k < B; k += 64) rs += W[(int64_t)i * B + k] + W[(int64_t)k * B + i];
    rs = wave_sum_f64(rs);
  }
  const bool project = g.normalize && s < 1e6;
  double dot = 0.0;
  if (project) {
    for (int t = lane; t < d; t += 64) {
      const double u = (double)xi[t] * s;
      const double gv = g.kind == XV_METRIC_SEMIHARD ? 2.0 * (rs * u - hv[t]) : hv[t];
      dot += gv * u;
    }
    dot = wave_sum_f64(dot);
  }
  float* out = ga.gx + (row0 + i) * ga.ldg;
  for (int t = lane; t < d; t += 64) {
    const double v = (double)xi[t] * s;            // s == 1 without `normalize`
    double gv = g.kind == XV_METRIC_SEMIHARD ? 2.0 * (rs * v - hv[t]) : hv[t];
    if (project) gv = gv - dot * v;
    if (g.normalize) gv = s * gv;
    out[t] = (float)(kappa * gv);
  }
}

struct GradLayout {
  int64_t panels, max_rows, rows;
  int64_t off_panels, off_scale, off_nrm, off_aux, off_slots, slot_bytes;
};

GradLayout grad_layout(int64_t num_groups, const int64_t* offsets, int d) {
  GradLayout l = {};
  for (int64_t g = 0; g < num_groups; ++g) {
    const int64_t b = offsets[g + 1] - offsets[g];
    l.max_rows = std::max(l.max_rows, b);
    l.panels += (b + kGAnchors - 1) / kGAnchors;
  }
  l.rows = offsets[num_groups];
  l.off_panels = round256(8 * (num_groups + 1));
  l.off_scale = l.off_panels + round256(8 * l.panels);
  l.off_nrm = l.off_scale + round256(8 * l.rows);
  l.off_aux = l.off_nrm + round256(8 * l.rows);
  l.off_slots = l.off_aux + round256(8 * l.rows);
  l.slot_bytes = round256(8 * l.max_rows * (l.max_rows + (int64_t)d));
  return l;
}

void free_grad_table(void* p) { delete static_cast<std::vector<int64_t>*>(p); }

}  // namespace

int64_t metric_loss_grad_workspace_bytes(int64_t num_groups, const int64_t* offsets, int d) {
  const GradLayout l = grad_layout(num_groups, offsets, d);
  return l.off_slots + l.slot_bytes;
}

hipError_t launch_metric_loss_grad(const float* x, int64_t ldx, const int64_t* offsets, int64_t num_groups, int d,
                                   const int32_t* labels, int kind, int pos_head, double margin, int squared, int normalize,
                                   double grad_scale, double* row_loss, int64_t* row_count, double* group_loss, int64_t* group_count,
                                   float* grad_x, int64_t ldg, void* ws, int64_t ws_bytes, hipStream_t stream) {
  const GradLayout l = grad_layout(num_groups, offsets, d);
  char* base = static_cast<char*>(ws);

  // the group and panel tables, one copy; freed in stream order behind it
  auto* table = new std::vector<int64_t>((size_t)(l.off_scale / 8), 0);
  std::copy(offsets, offsets + num_groups + 1, table->begin());
  std::vector<int64_t> first_panel((size_t)num_groups + 1, 0);
  {
    int32_t* pt = reinterpret_cast<int32_t*>(table->data() + l.off_panels / 8);
    for (int64_t g = 0; g < num_groups; ++g) {
      for (int64_t a = 0; a < offsets[g + 1] - offsets[g]; a += kGAnchors) {
        *pt++ = (int32_t)g;
        *pt++ = (int32_t)a;
      }
      first_panel[(size_t)g + 1] = first_panel[(size_t)g] + (offsets[g + 1] - offsets[g] + kGAnchors - 1) / kGAnchors;
    }
  }
  hipError_t e = hipMemcpyAsync(ws, table->data(), (size_t)l.off_scale, hipMemcpyHostToDevice, stream);

  GradArgs ga = {};
  MetricArgs& a = ga.m;
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
  a.row_loss = row_loss;
  a.row_count = row_count;
  a.group_loss = group_loss;
  a.group_count = group_count;
  a.max_rows = (int)l.max_rows;
  a.vec = (ldx & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  ga.slots = reinterpret_cast<double*>(base + l.off_slots);
  ga.slot_doubles = l.slot_bytes / 8;
  ga.gx = grad_x;
  ga.ldg = ldg;
  ga.grad_scale = grad_scale;

  if (e == hipSuccess) {
    const int64_t r0 = offsets[0], r1 = offsets[num_groups];
    hipLaunchKernelGGL(row_stats_kernel, dim3((unsigned)((r1 - r0 + 63) / 64)), dim3(256), 0, stream, a, r0, r1);
    e = hipGetLastError();
  }
  const size_t lds = (size_t)((l.max_rows + 1) / 2) * sizeof(double) + (size_t)kGAnchors * (size_t)(l.max_rows | 1) * sizeof(double) +
                     (size_t)kGAnchors * (size_t)l.max_rows * sizeof(int32_t);
  if (e == hipSuccess) {
    static std::mutex mu;            // per-device attribute; any thread may make the first launch on a device
    static bool set_for[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    std::lock_guard<std::mutex> lock(mu);
    if (!set_for[dev & 63]) {
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(grad_panel_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(kGradMaxRows / 2 * sizeof(double) + kGAnchors * (kGradMaxRows | 1) * sizeof(double) +
                                    kGAnchors * kGradMaxRows * sizeof(int32_t)));
      if (e == hipSuccess) set_for[dev & 63] = true;
    }
  }
  const int64_t slots = std::max<int64_t>(std::min<int64_t>((ws_bytes - l.off_slots) / l.slot_bytes, kGradMaxSlots), 1);
  const int tiles = (int)((l.max_rows + 15) / 16);
  for (int64_t g0 = 0; g0 < num_groups && e == hipSuccess; g0 += slots) {
    const int64_t g1 = std::min(g0 + slots, num_groups);
    ga.g0 = g0;
    ga.ngroups = (int)(g1 - g0);
    ga.p0 = first_panel[(size_t)g0];
    ga.p1 = first_panel[(size_t)g1];
    hipLaunchKernelGGL(grad_panel_kernel, dim3((unsigned)(ga.p1 - ga.p0)), dim3(kGThreads), lds, stream, ga);
    e = hipGetLastError();
    if (e == hipSuccess) {
      hipLaunchKernelGGL(hv_kernel, dim3((unsigned)(ga.ngroups * tiles), (unsigned)((d + 16 * kGWaves - 1) / (16 * kGWaves))),
                         dim3(kGThreads), 0, stream, ga);
      e = hipGetLastError();
    }
    if (e == hipSuccess) {
      hipLaunchKernelGGL(grad_rows_kernel, dim3((unsigned)ga.ngroups, (unsigned)((l.max_rows + kGWaves - 1) / kGWaves)),
                         dim3(kGThreads), 0, stream, ga);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)((num_groups + 63) / 64)), dim3(64), 0, stream, a);
    e = hipGetLastError();
  }
  if (hipLaunchHostFunc(stream, free_grad_table, table) != hipSuccess) {
    (void)hipStreamSynchronize(stream);
    delete table;
  }
  return e;
}

}  // namespace xv
