// Speaker clustering (include/xvec_hip.h, xv_ahc): average-linkage agglomerative clustering of the rows of one recording from
// its dense score matrix, what Kaldi's diarization/cluster.sh does with agglomerative-cluster.  The reference has no
// clustering step: **parity unpinned**; the rule is stated in the header and restated in numpy by tests/helpers/ref_cluster.py.
//
// One 256-thread workgroup clusters one group; groups never wait for each other, __syncthreads is the only synchronisation,
// and there is no atomic of any kind.  Only the upper triangle of a group's matrix is read or written: S(x, y) of two live
// clusters x < y lives at s[x * ld + y] all the way through.
//
// State in LDS, 16 bytes per row: key[r] / partner[r] = the row-best cache (the largest linkage L(r, k) over the live k > r and
// the lowest k that attains it; partner -1: no such k, or r is dead; -2: to be recomputed) and size[r] (0: dead).  A step is
//   1. a reduction over the cache: largest key, lowest row among equal keys (the cached partner is already the lowest column);
//   2. the merge of b into a: one thread per live k adds S(b, k) to S(a, k) -- one float32 addition, so every sum is the chain
//      of additions that the merge order fixes, whatever the thread layout -- and looks at the cache of row k: a row whose
//      partner was a or b is marked, a row k < a takes a as its partner if the changed column now beats (or ties below) its
//      cached one, rows above a keep their cache because nothing to their right changed except the death of b;
//   3. a recompute of the marked rows (always a), one wave per row.
// Steps 1 and 2 cost O(n / 256) per thread; without the cache every step would rescan the triangle, O(n^3) per recording.
// The loop is a for over at most n - 1 steps: the bound is the counter, never a data condition.
//
// Linkage: L = double(S) / double(int64 |A| * |B|), one IEEE double division (hipcc's default division is correctly rounded).
//
// Error of the float32 sums.  S(A, B) is the sum of the |A| |B| original scores of the member pairs, accumulated by one float32
// addition per merge that touched A or B: a binary tree with |A| |B| leaves whose depth is at most the number of merges, and a
// group performs at most n - 1 merges of which the last produces no sum that is used, so a leaf passes through at most n - 2
// additions.  With u = 2^-24 each addition multiplies what it carries by (1 + e), |e| <= u, so
//   |S - exact sum| <= ((1 + u)^(n - 2) - 1) sum |s| <= (n - 2) u (1 + (n - 2) u) |A| |B| max|s|      (n u < 2^-11 for n <= 8192)
// and after the division by |A| |B| (relative error 2^-53, inside the "small" below)
//   |L - exact mean| <= (n - 2) 2^-24 (1 + small) max|s|,   small < 2^-10.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "xv_kernels.h"

namespace xv {
namespace {

struct AhcGroup {       // one group as the kernel sees it (32 bytes; an array of these is the whole workspace)
  int64_t s_off;        // float offset of the group's matrix in s
  int64_t out_off;      // offset of its slots in labels / merge_a / merge_b / merge_height
  int32_t n;
  int32_t target;
  int32_t group;        // its number in the caller's order (index of num_clusters)
  int32_t pad;
};

struct Best {
  double l;
  int a, b;             // a < 0: none
};

// x is replaced by y when y is the better pair: larger linkage, then lower row, then lower column
__device__ __forceinline__ bool better(const Best& y, const Best& x) {
  if (y.a < 0) return false;
  if (x.a < 0) return true;
  if (y.l != x.l) return y.l > x.l;
  if (y.a != x.a) return y.a < x.a;
  return y.b < x.b;
}

__device__ __forceinline__ Best wave_best(Best v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    Best o;
    o.l = __shfl_xor(v.l, off, 64);
    o.a = __shfl_xor(v.a, off, 64);
    o.b = __shfl_xor(v.b, off, 64);
    if (better(o, v)) v = o;
  }
  return v;
}

// the row-best cache of row r, by one wave: lanes take the columns k > r in turn (ascending per lane, so a strict > keeps the
// lowest column of a lane) and the wave reduction breaks ties to the lowest column
__device__ void row_best(const float* srow, int r, int n, const int* size, double* key, int* partner, int lane) {
  const long long sr = size[r];
  Best v{0.0, -1, -1};
  for (int k = r + 1 + lane; k < n; k += 64) {
    const int sk = size[k];
    if (sk > 0) {
      const double l = (double)srow[k] / (double)(sr * (long long)sk);
      if (l == l && (v.a < 0 || l > v.l)) { v.l = l; v.a = r; v.b = k; }
    }
  }
  v = wave_best(v);
  if (lane == 0) {
    key[r] = v.l;
    partner[r] = v.a < 0 ? -1 : v.b;
  }
}

__global__ __launch_bounds__(256) void ahc_kernel(float* __restrict__ s_all, const AhcGroup* __restrict__ groups, double threshold,
                                                  int32_t* __restrict__ labels_all, int32_t* __restrict__ num_clusters,
                                                  int32_t* __restrict__ merge_a_all, int32_t* __restrict__ merge_b_all,
                                                  double* __restrict__ merge_height_all) {
  extern __shared__ double lds[];
  __shared__ Best red[4];
  __shared__ int scan[256];
  const AhcGroup g = groups[blockIdx.x];
  const int n = g.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (n == 0) {
    if (tid == 0) num_clusters[g.group] = 0;
    return;
  }
  const int64_t ld = n < 4 ? 4 : (int64_t)((n + 3) & ~3);
  float* s = s_all + g.s_off;
  int32_t* labels = labels_all + g.out_off;             // the parent of every row while the loop runs
  int32_t* merge_a = merge_a_all + g.out_off;
  int32_t* merge_b = merge_b_all + g.out_off;
  double* merge_height = merge_height_all + g.out_off;
  double* key = lds;
  int* partner = reinterpret_cast<int*>(key + n);
  int* size = partner + n;

  for (int r = tid; r < n; r += 256) {
    size[r] = 1;
    partner[r] = -2;
    labels[r] = r;
  }
  __syncthreads();
  int redo = n;                  // rows [0, redo) may carry the mark
  int merges = 0;
  for (int step = 0; step < n; ++step) {          // passes 0 .. n - 2 merge at most once each; pass n - 1 only stops
    // ---- 3 (of the previous step; all rows before the first): recompute the marked rows, 64-row chunks dealt to the waves
    for (int c = wave; c * 64 < redo; c += 4) {
      const int r0 = c * 64 + lane;
      unsigned long long mask = __ballot(r0 < redo && partner[r0] == -2);
      for (int it = 0; it < 64 && mask; ++it) {
        const int j = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const int r = c * 64 + j;
        row_best(s + (int64_t)r * ld, r, n, size, key, partner, lane);
      }
    }
    __syncthreads();
    if (n - merges <= g.target || step == n - 1) break;
    // ---- 1: the best pair of the cache
    Best v{0.0, -1, -1};
    for (int r = tid; r < n; r += 256) {
      const int p = partner[r];
      if (p >= 0) {
        const double l = key[r];
        if (v.a < 0 || l > v.l) { v.l = l; v.a = r; v.b = p; }
      }
    }
    v = wave_best(v);
    if (lane == 0) red[wave] = v;
    __syncthreads();
    v = red[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (better(red[w], v)) v = red[w];
    if (v.a < 0 || !(v.l >= threshold)) break;         // uniform: every thread holds the same v
    // ---- 2: merge b into a
    const int a = v.a, b = v.b;
    const long long sab = (long long)size[a] + size[b];
    __syncthreads();                                   // every thread has read red and the two sizes
    if (tid == 0) {
      size[a] = (int)sab;
      size[b] = 0;
      partner[a] = -2;
      partner[b] = -1;
      labels[b] = a;
      merge_a[merges] = a;
      merge_b[merges] = b;
      merge_height[merges] = v.l;
    }
    for (int k = tid; k < n; k += 256) {
      if (k == a || k == b) continue;
      const int sk = size[k];
      if (sk == 0) continue;
      float* pa = k < a ? s + (int64_t)k * ld + a : s + (int64_t)a * ld + k;
      const float* pb = k < b ? s + (int64_t)k * ld + b : s + (int64_t)b * ld + k;
      const float sum = *pa + *pb;
      *pa = sum;
      if (k > b) continue;                             // nothing to the right of row k changed
      const int p = partner[k];
      if (p == a || p == b) {
        partner[k] = -2;
      } else if (k < a) {
        const double l = (double)sum / (double)((long long)sk * sab);
        if (l == l && (p < 0 || l > key[k] || (l == key[k] && a < p))) {
          key[k] = l;
          partner[k] = a;
        }
      }
    }
    ++merges;
    redo = b;                                          // a < b, and only rows below b can be marked
    __syncthreads();
  }
  __syncthreads();
  // ---- the unused slots of the log, the count, and the labels: clusters numbered by their lowest row
  for (int i = merges + tid; i < n; i += 256) {
    merge_a[i] = -1;
    merge_b[i] = -1;
    merge_height[i] = __longlong_as_double(0x7ff8000000000000ll);
  }
  if (tid == 0) num_clusters[g.group] = n - merges;
  for (int i = tid; i < n; i += 256) {                 // parent chains fall strictly, so n hops are enough
    int r = i;
    for (int hop = 0; hop < n; ++hop) {
      const int p = labels[r];
      if (p == r) break;
      r = p;
    }
    partner[i] = r;
  }
  const int per = (n + 255) / 256, lo = min(n, tid * per), hi = min(n, lo + per);
  int roots = 0;
  for (int i = lo; i < hi; ++i) roots += size[i] > 0;
  scan[tid] = roots;
  __syncthreads();                                     // also: every chain has been followed before a label is overwritten
  int before = 0;
  for (int t = 0; t < tid; ++t) before += scan[t];
  int* rank = reinterpret_cast<int*>(key);
  for (int i = lo; i < hi; ++i)
    if (size[i] > 0) rank[i] = before++;
  __syncthreads();
  for (int i = tid; i < n; i += 256) labels[i] = rank[partner[i]];
}

}  // namespace

int64_t ahc_matrix_floats(int64_t n) { return n <= 0 ? 0 : n * std::max<int64_t>(4, (n + 3) / 4 * 4); }

int64_t ahc_workspace_bytes(int64_t num_groups) { return (num_groups * (int64_t)sizeof(AhcGroup) + 255) / 256 * 256; }

static void free_group_table(void* p) { delete static_cast<std::vector<AhcGroup>*>(p); }

hipError_t launch_ahc(float* s, const int32_t* rows, const int32_t* target, int64_t num_groups, double threshold, int32_t* labels,
                      int32_t* num_clusters, int32_t* merge_a, int32_t* merge_b, double* merge_height, void* ws, hipStream_t stream) {
  auto* table = new std::vector<AhcGroup>((size_t)num_groups);
  std::vector<AhcGroup>& desc = *table;
  int64_t s_off = 0, out_off = 0;
  int nmax = 0;
  for (int64_t g = 0; g < num_groups; ++g) {
    desc[g] = AhcGroup{s_off, out_off, rows[g], target ? target[g] : 1, (int32_t)g, 0};
    s_off += ahc_matrix_floats(rows[g]);
    out_off += rows[g];
    nmax = std::max(nmax, (int)rows[g]);
  }
  // large groups first: the longest workgroups start in the first wave of the grid instead of trailing it
  std::stable_sort(desc.begin(), desc.end(), [](const AhcGroup& x, const AhcGroup& y) { return x.n > y.n; });
  hipError_t e = hipMemcpyAsync(ws, desc.data(), desc.size() * sizeof(AhcGroup), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) {
    static std::mutex mu;            // per-device attribute; any thread may make the first launch on a device
    static size_t set_for[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    std::lock_guard<std::mutex> lock(mu);
    if (!set_for[dev & 63]) {        // the cache of the largest legal group: 8192 rows x 16 bytes = 128 KiB of the CU's 160
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(ahc_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 8192 * 16);
      if (e == hipSuccess) set_for[dev & 63] = 1;
    }
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(ahc_kernel, dim3((unsigned)num_groups), dim3(256), (size_t)std::max(nmax, 1) * 16, stream, s,
                       static_cast<const AhcGroup*>(ws), threshold, labels, num_clusters, merge_a, merge_b, merge_height);
    e = hipGetLastError();
  }
  // the copy may still be reading the table when this returns: it is freed in stream order, behind the copy
  if (hipLaunchHostFunc(stream, free_group_table, table) != hipSuccess) {
    (void)hipStreamSynchronize(stream);
    delete table;
  }
  return e;
}

}  // namespace xv
