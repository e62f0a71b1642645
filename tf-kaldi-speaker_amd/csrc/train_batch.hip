// The batch former of training: one launch turns the staged record bytes of a batch (csrc/train_stage.cpp) into the packed
// float32 batch [B * length, dim] the trainers take.  The rule is in include/xvec_hip.h (xv_train_batch_decode); for 'CM '
// records it restates read_payload of csrc/ark_io.cpp, the oracle of tests/test_gpu_train_batch.py: bit equality, element by
// element.
//
// How the arithmetic rounds as the host's does.
//  * The host code is plain C++ doubles on x86-64: every *, /, +, - rounds once, nothing is fused.  This translation unit is
//    compiled with `#pragma clang fp contract(off)` (device code defaults to contract(fast), which would turn p + s * v into one
//    v_fma_f64 and change the last bit), no fast-math flag, and uses no intrinsic: the products and sums below are separate
//    v_mul_f64 / v_add_f64.
//  * (p1 - p0) / 64 and / 128 are exact scalings whichever way they are written.  / 63 is the compiler's IEEE double division
//    (v_div_scale / v_rcp / v_fma / v_div_fmas / v_div_fixup: correctly rounded, no approximation flag is set).  The three slopes
//    depend on the column alone, so they are computed once per column and tile, not per element: the same operation on the same
//    operands gives the same double.
//  * uint16 -> double, byte -> double and the int differences v - 64, v - 192 are exact.  double -> float is v_cvt_f32_f64,
//    round-to-nearest-even with float32 denormals kept (the default float mode of a HIP kernel), like the host's cvtsd2ss.
//
// The shape.  A workgroup of 256 threads owns one tile of at most 64 rows x 64 columns of one chunk.  'CM ' payloads are
// column-major bytes: lanes run along the rows of a column (64 consecutive bytes per wave), the decoded floats go through a
// [64][65] LDS tile and leave with lanes along the columns of a row, so both sides are coalesced.  'FM ' / 'DM ' payloads are
// row-major already and are copied / rounded with the output's lane mapping.  With dim <= 32 a wave covers 64 / cw rows of
// cw = the next power of two >= the tile's width, so a 30-column batch keeps 60 of 64 lanes busy.  Memory-bound and small
// (0.6 MB in, 2.3 MB out for 64 x 300 x 30); nothing is scheduled by hand.
#include "xv_model.h"

#pragma clang fp contract(off)

using namespace xv;
using namespace xv::api;

namespace {

constexpr int kTile = 64;
constexpr int kThreads = 256;

struct ColLine { double p0, p1, p2, s0, s1, s2; };    // a column's percentiles 0..2 and the slopes of its three pieces

__global__ __launch_bounds__(kThreads) void train_batch_decode_kernel(const unsigned char* __restrict__ staged,
                                                                      const xv_train_chunk* __restrict__ chunks, int length,
                                                                      int dim, int row_tiles, int col_tiles, float* __restrict__ out,
                                                                      int64_t ld) {
  __shared__ float tile[kTile][kTile + 1];
  __shared__ ColLine lines[kTile];
  const int per_chunk = row_tiles * col_tiles;
  const int chunk = (int)(blockIdx.x / (unsigned)per_chunk);
  const int in_chunk = (int)(blockIdx.x - (unsigned)chunk * (unsigned)per_chunk);
  const int r0 = (in_chunk / col_tiles) * kTile, c0 = (in_chunk % col_tiles) * kTile;
  const int th = min(kTile, length - r0), tw = min(kTile, dim - c0);
  const xv_train_chunk d = chunks[chunk];
  const int t = (int)threadIdx.x;
  // lanes along the columns of a row: cw = the power of two >= tw, 256 / cw rows per pass
  int cs = 0;
  while ((1 << cs) < tw) ++cs;
  const int oc = t & ((1 << cs) - 1), orow = t >> cs, ostep = kThreads >> cs;
  float* const obase = out + ((int64_t)chunk * length + r0) * ld + c0;

  if (d.kind == XV_TRAIN_CM) {
    if (t < tw) {
      const uint16_t* h = reinterpret_cast<const uint16_t*>(staged + d.header_off) + 4 * (int64_t)(c0 + t);
      const double gmin = d.gmin, grange = d.grange;
      double p[4];
      for (int i = 0; i < 4; ++i) p[i] = (double)(float)(gmin + grange * 1.52590218966964e-05 * (double)h[i]);
      ColLine l;
      l.p0 = p[0];
      l.p1 = p[1];
      l.p2 = p[2];
      l.s0 = (p[1] - p[0]) / 64.;
      l.s1 = (p[2] - p[1]) / 128.;
      l.s2 = (p[3] - p[2]) / 63.;
      lines[t] = l;
    }
    __syncthreads();
    const int r = t & (kTile - 1);
    if (r < th) {
      const unsigned char* col = staged + d.payload_off + (int64_t)d.first_row + r0 + r;
      for (int c = t >> 6; c < tw; c += kThreads / kTile) {
        const int v = col[(int64_t)(c0 + c) * d.rows];
        const ColLine l = lines[c];
        double x;
        if (v <= 64) x = l.p0 + l.s0 * v;
        else if (v <= 192) x = l.p1 + l.s1 * (v - 64);
        else x = l.p2 + l.s2 * (v - 192);
        tile[c][r] = (float)x;
      }
    }
    __syncthreads();
    if (oc < tw)
      for (int r2 = orow; r2 < th; r2 += ostep) obase[(int64_t)r2 * ld + oc] = tile[oc][r2];
  } else if (d.kind == XV_TRAIN_FM) {
    const float* src = reinterpret_cast<const float*>(staged + d.payload_off) + ((int64_t)d.first_row + r0) * d.cols + c0;
    if (oc < tw)
      for (int r2 = orow; r2 < th; r2 += ostep) obase[(int64_t)r2 * ld + oc] = src[(int64_t)r2 * d.cols + oc];
  } else {
    const double* src = reinterpret_cast<const double*>(staged + d.payload_off) + ((int64_t)d.first_row + r0) * d.cols + c0;
    if (oc < tw)
      for (int r2 = orow; r2 < th; r2 += ostep) obase[(int64_t)r2 * ld + oc] = (float)src[(int64_t)r2 * d.cols + oc];
  }
}

void free_chunks(void* p) { delete static_cast<std::vector<xv_train_chunk>*>(p); }

}  // namespace

extern "C" {

int64_t xv_train_batch_workspace(int64_t num_chunks) {
  if (num_chunks < 0 || num_chunks >= ((int64_t)1 << 31)) return XV_ERR_INVALID;
  return (num_chunks * (int64_t)sizeof(xv_train_chunk) + 255) & ~(int64_t)255;
}

int xv_train_batch_decode(int device, const void* staged_dev, int64_t staged_bytes, const xv_train_chunk* chunks_host,
                          int64_t num_chunks, int length, int dim, float* out_dev, int64_t ld, void* ws_dev, int64_t ws_bytes,
                          void* stream) {
  const char* op = "xv_train_batch_decode";
  if (!staged_dev || !chunks_host || !out_dev || !ws_dev) return fail(nullptr, XV_ERR_INVALID, "%s: null pointer", op);
  if (num_chunks < 1 || length < 1 || dim < 1 || ld < dim || staged_bytes < 0)
    return fail(nullptr, XV_ERR_INVALID, "%s: bad dimensions (num_chunks %lld, length %d, dim %d, ld %lld)", op, (long long)num_chunks,
                length, dim, (long long)ld);
  const int64_t row_tiles = ((int64_t)length + kTile - 1) / kTile, col_tiles = ((int64_t)dim + kTile - 1) / kTile;
  if (num_chunks >= ((int64_t)1 << 31) || num_chunks * row_tiles * col_tiles >= ((int64_t)1 << 31))
    return fail(nullptr, XV_ERR_INVALID, "%s: %lld chunks of %d x %d are more than 2^31 tiles", op, (long long)num_chunks, length, dim);
  for (int64_t i = 0; i < num_chunks; ++i) {
    const xv_train_chunk& c = chunks_host[i];
    const char* what = nullptr;
    if (c.kind != XV_TRAIN_FM && c.kind != XV_TRAIN_DM && c.kind != XV_TRAIN_CM) what = "unknown kind";
    else if (c.cols < 1) what = "cols < 1";
    else if (dim > c.cols) what = "dim > cols";
    else if (c.first_row < 0 || c.rows < 1 || (int64_t)c.first_row + length > c.rows) what = "first_row + length > staged rows";
    else if (c.payload_off < 0 || (c.payload_off & 15)) what = "payload offset is not a multiple of 16";
    else {
      const int64_t es = c.kind == XV_TRAIN_FM ? 4 : (c.kind == XV_TRAIN_DM ? 8 : 1);
      const int64_t cells = (int64_t)c.rows * c.cols;                      // below 2^62: both are int32
      if (cells > ((int64_t)1 << 56) || c.payload_off > staged_bytes || cells * es > staged_bytes - c.payload_off)
        what = "payload reaches past the staged bytes";
      else if (c.kind == XV_TRAIN_CM &&
               (c.header_off < 0 || (c.header_off & 7) || c.header_off > staged_bytes || (int64_t)c.cols * 8 > staged_bytes - c.header_off))
        what = "column headers misaligned or past the staged bytes";
    }
    if (what) return fail(nullptr, XV_ERR_INVALID, "%s: chunk %lld: %s", op, (long long)i, what);
  }
  const int64_t need = xv_train_batch_workspace(num_chunks);
  if (ws_bytes < need) return fail(nullptr, XV_ERR_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", op, (long long)ws_bytes, (long long)need);
  DeviceGuard g(device);
  if (!g.ok) return fail(nullptr, XV_ERR_HIP, "cannot select HIP device %d", device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the copy may still be reading the table when this returns: a private copy of it is freed in stream order, behind the copy
  auto* table = new (std::nothrow) std::vector<xv_train_chunk>(chunks_host, chunks_host + num_chunks);
  if (!table) return fail(nullptr, XV_ERR_HIP, "%s: out of host memory", op);
  hipError_t e = hipMemcpyAsync(ws_dev, table->data(), (size_t)num_chunks * sizeof(xv_train_chunk), hipMemcpyHostToDevice, s);
  if (hipLaunchHostFunc(s, free_chunks, table) != hipSuccess) {
    (void)hipStreamSynchronize(s);
    delete table;
  }
  if (e != hipSuccess) return fail(nullptr, XV_ERR_HIP, "%s: descriptor upload failed: %s", op, hipGetErrorString(e));
  hipLaunchKernelGGL(train_batch_decode_kernel, dim3((unsigned)(num_chunks * row_tiles * col_tiles)), dim3(kThreads), 0, s,
                     static_cast<const unsigned char*>(staged_dev), static_cast<const xv_train_chunk*>(ws_dev), length, dim,
                     (int)row_tiles, (int)col_tiles, out_dev, ld);
  e = hipGetLastError();
  if (e != hipSuccess) return fail(nullptr, XV_ERR_HIP, "%s launch failed: %s", op, hipGetErrorString(e));
  return XV_OK;
}

}  // extern "C"
