// C ABI of libxvec_hip.so, the stateless ops: front-end, scoring, PLDA, back-end statistics, loss heads (classifier and metric), clustering
// and calibration.  Every wrapper validates its arguments and hands one launch (or a short chain) to with_device().
#include <cfloat>

#include "xv_model.h"

using namespace xv;
using namespace xv::api;

namespace {

hipStream_t to_stream(void* stream) { return static_cast<hipStream_t>(stream); }

// The common tail of every device wrapper: select `device` (the caller's current device is restored on return), run `launch`
// and turn its hipError_t into the op's message.
template <class Launch>
int with_device(int device, const char* op, Launch&& launch) {
  DeviceGuard g(device);
  if (!g.ok) return fail(nullptr, XV_ERR_HIP, "cannot select HIP device %d", device);
  const hipError_t e = launch();
  if (e != hipSuccess) return fail(nullptr, XV_ERR_HIP, "%s launch failed: %s", op, hipGetErrorString(e));
  return XV_OK;
}

}  // namespace


extern "C" {

int xv_frontend_cmn_select(int device, const float* feats_dev, int ld, int dim, const int32_t* frame_offsets_dev,
                           int batch, const int32_t* src_rows_dev, int64_t out_rows, int cmn_window, int center,
                           int min_window, double* scratch_dev, float* out_dev, void* stream) {
  if (!feats_dev || !frame_offsets_dev || !src_rows_dev || !scratch_dev || !out_dev)
    return fail(nullptr, XV_ERR_INVALID, "xv_frontend_cmn_select: null pointer");
  if (dim < 1 || dim > 1024 || ld < dim || batch < 1 || out_rows < 0 || cmn_window < 0)
    return fail(nullptr, XV_ERR_INVALID, "xv_frontend_cmn_select: bad dimensions");
  return with_device(device, "cmn_select", [&] {
    return launch_cmn_select(feats_dev, ld, dim, frame_offsets_dev, batch, scratch_dev, src_rows_dev, out_rows,
                             cmn_window, center, min_window, out_dev, to_stream(stream));
  });
}

int xv_mfcc_create(const xv_mfcc_opts* opts, int device, xv_mfcc** out) {
  if (!opts || !out) return fail(nullptr, XV_ERR_INVALID, "xv_mfcc_create: null pointer");
  *out = nullptr;
  std::string err;
  const int rc = mfcc_create(opts, device, out, &err);
  if (rc != XV_OK) return fail(nullptr, rc, "xv_mfcc_create: %s", err.c_str());
  return XV_OK;
}

void xv_mfcc_destroy(xv_mfcc* m) { mfcc_destroy(m); }

int64_t xv_mfcc_num_frames(const xv_mfcc* m, int64_t num_samples) {
  int64_t t = 0;
  if (!m || mfcc_num_frames(m, num_samples, &t) != 0) return fail(nullptr, XV_ERR_INVALID, "xv_mfcc_num_frames: bad argument");
  return t;
}

int xv_mfcc_compute(xv_mfcc* m, const int16_t* wave_dev, const int64_t* sample_offsets_dev, const int32_t* frame_offsets_dev,
                    int batch, float* feats_dev, int64_t ld, void* stream) {
  if (!m || !wave_dev || !sample_offsets_dev || !frame_offsets_dev || !feats_dev)
    return fail(nullptr, XV_ERR_INVALID, "xv_mfcc_compute: null pointer");
  if (batch < 1 || ld < mfcc_num_ceps(m)) return fail(nullptr, XV_ERR_INVALID, "xv_mfcc_compute: bad dimensions (batch >= 1, ld >= num_ceps)");
  return with_device(mfcc_device(m), "mfcc", [&] {
    return launch_mfcc(m, wave_dev, sample_offsets_dev, frame_offsets_dev, batch, feats_dev, ld,
                       to_stream(stream));
  });
}

int xv_vad_energy(int device, const float* feats_dev, int64_t ld, const int32_t* frame_offsets_dev, int batch, float threshold,
                  float mean_scale, int context, float proportion, float* vad_dev, void* stream) {
  if (!feats_dev || !frame_offsets_dev || !vad_dev) return fail(nullptr, XV_ERR_INVALID, "xv_vad_energy: null pointer");
  if (batch < 1 || ld < 1 || context < 0 || !(proportion >= 0.f && proportion <= 1.f))
    return fail(nullptr, XV_ERR_INVALID, "xv_vad_energy: bad arguments (batch >= 1, ld >= 1, context >= 0, 0 <= proportion <= 1)");
  return with_device(device, "vad", [&] {
    return launch_vad_energy(feats_dev, ld, frame_offsets_dev, batch, threshold, mean_scale, context, proportion,
                             vad_dev, to_stream(stream));
  });
}

int xv_fbank_create(const xv_fbank_opts* opts, int device, xv_fbank** out) {
  if (!opts || !out) return fail(nullptr, XV_ERR_INVALID, "xv_fbank_create: null pointer");
  *out = nullptr;
  std::string err;
  const int rc = fbank_create(opts, device, out, &err);
  if (rc != XV_OK) return fail(nullptr, rc, "xv_fbank_create: %s", err.c_str());
  return XV_OK;
}

void xv_fbank_destroy(xv_fbank* m) { fbank_destroy(m); }

int64_t xv_fbank_num_frames(const xv_fbank* m, int64_t num_samples) {
  int64_t t = 0;
  if (!m || fbank_num_frames(m, num_samples, &t) != 0) return fail(nullptr, XV_ERR_INVALID, "xv_fbank_num_frames: bad argument");
  return t;
}

int xv_fbank_num_feats(const xv_fbank* m) {
  if (!m) return fail(nullptr, XV_ERR_INVALID, "xv_fbank_num_feats: null pointer");
  return fbank_num_feats(m);
}

int xv_fbank_compute(xv_fbank* m, const int16_t* wave_dev, const int64_t* sample_offsets_dev, const int32_t* frame_offsets_dev,
                     int batch, float* feats_dev, int64_t ld, float* log_energy_dev, void* stream) {
  if (!m || !wave_dev || !sample_offsets_dev || !frame_offsets_dev || !feats_dev)
    return fail(nullptr, XV_ERR_INVALID, "xv_fbank_compute: null pointer");
  if (batch < 1 || ld < fbank_num_feats(m)) return fail(nullptr, XV_ERR_INVALID, "xv_fbank_compute: bad dimensions (batch >= 1, ld >= num_feats)");
  return with_device(fbank_device(m), "fbank", [&] {
    return launch_fbank(m, wave_dev, sample_offsets_dev, frame_offsets_dev, batch, feats_dev, ld, log_energy_dev,
                        to_stream(stream));
  });
}

int xv_length_normalize(int device, const float* x_dev, int64_t ldx, int64_t rows, int dim, int scaleup, float* out_dev,
                        int64_t ldo, void* stream) {
  if (!x_dev || !out_dev) return fail(nullptr, XV_ERR_INVALID, "xv_length_normalize: null pointer");
  if (rows < 0 || dim < 1 || ldx < dim || ldo < dim) return fail(nullptr, XV_ERR_INVALID, "xv_length_normalize: bad dimensions");
  return with_device(device, "length_norm", [&] {
    return launch_length_norm(x_dev, ldx, rows, dim, scaleup, out_dev, ldo, to_stream(stream));
  });
}

int xv_speaker_mean(int device, const float* x_dev, int64_t ldx, int dim, const int32_t* spk_offsets_dev,
                    const int32_t* utt_index_dev, int64_t num_speakers, float* out_dev, int64_t ldo, void* stream) {
  if (!x_dev || !out_dev || !spk_offsets_dev || !utt_index_dev) return fail(nullptr, XV_ERR_INVALID, "xv_speaker_mean: null pointer");
  if (num_speakers < 0 || dim < 1 || ldx < dim || ldo < dim) return fail(nullptr, XV_ERR_INVALID, "xv_speaker_mean: bad dimensions");
  return with_device(device, "speaker_mean", [&] {
    return launch_speaker_mean(x_dev, ldx, dim, spk_offsets_dev, utt_index_dev, num_speakers, out_dev, ldo,
                               to_stream(stream));
  });
}

// shared argument check of the two Gram entry points
static int gram_operands(const char* who, const void* x, int64_t ldx, int64_t n, int d, const double* g, const void* ws,
                         int64_t ws_bytes) {
  if (d < 1 || d > 2048) return fail(nullptr, XV_ERR_UNSUPPORTED, "%s: 1 <= d <= 2048, got %d", who, d);
  if (n < 0 || ldx < d || !g || (n > 0 && !x)) return fail(nullptr, XV_ERR_INVALID, "%s: bad arguments", who);
  const int64_t need = gram_f64_workspace_bytes(n, d);
  if (ws_bytes < need || (need > 0 && !ws))
    return fail(nullptr, XV_ERR_WORKSPACE, "%s: workspace %lld bytes < %lld", who, (long long)ws_bytes, (long long)need);
  return XV_OK;
}

int64_t xv_gram_f64_workspace(int64_t n, int d) {
  if (d < 1 || d > 2048) return fail(nullptr, XV_ERR_UNSUPPORTED, "xv_gram_f64_workspace: 1 <= d <= 2048, got %d", d);
  if (n < 0) return fail(nullptr, XV_ERR_INVALID, "xv_gram_f64_workspace: n < 0");
  return gram_f64_workspace_bytes(n, d);
}

int xv_gram_f64(int device, const float* x_dev, int64_t ldx, int64_t n, int d, const double* c_dev, const double* w_dev,
                double* g_dev, void* ws_dev, int64_t ws_bytes, void* stream) {
  if (const int rc = gram_operands("xv_gram_f64", x_dev, ldx, n, d, g_dev, ws_dev, ws_bytes)) return rc;
  return with_device(device, "gram_f64", [&] {
    return launch_gram_f64(x_dev, ldx, n, d, c_dev, w_dev, g_dev, static_cast<double*>(ws_dev),
                           to_stream(stream));
  });
}

int xv_gram_f64_rows64(int device, const double* x_dev, int64_t ldx, int64_t n, int d, const double* c_dev, const double* w_dev,
                       double* g_dev, void* ws_dev, int64_t ws_bytes, void* stream) {
  if (const int rc = gram_operands("xv_gram_f64_rows64", x_dev, ldx, n, d, g_dev, ws_dev, ws_bytes)) return rc;
  return with_device(device, "gram_f64_rows64", [&] {
    return launch_gram_f64_rows64(x_dev, ldx, n, d, c_dev, w_dev, g_dev, static_cast<double*>(ws_dev),
                                  to_stream(stream));
  });
}

int xv_class_mean_f64(int device, const float* x_dev, int64_t ldx, int64_t n, int dim, const int32_t* spk_offsets_dev,
                      const int32_t* utt_index_dev, int64_t num_classes, const double* c_dev, double* out_dev, int64_t ldo,
                      void* stream) {
  if (!x_dev || !out_dev || !spk_offsets_dev || !utt_index_dev) return fail(nullptr, XV_ERR_INVALID, "xv_class_mean_f64: null pointer");
  if (num_classes < 0 || n < 0 || dim < 1 || ldx < dim || ldo < dim) return fail(nullptr, XV_ERR_INVALID, "xv_class_mean_f64: bad dimensions");
  return with_device(device, "class_mean_f64", [&] {
    return launch_class_mean_f64(x_dev, ldx, n, dim, spk_offsets_dev, utt_index_dev, num_classes, c_dev, out_dev, ldo,
                                 to_stream(stream));
  });
}

int xv_reverb_tile(int* tile, int* chunk) {
  if (!tile || !chunk) return fail(nullptr, XV_ERR_INVALID, "xv_reverb_tile: null pointer");
  *tile = XV_REVERB_TILE;
  *chunk = XV_REVERB_CHUNK;
  return XV_OK;
}

int64_t xv_reverb_workspace(const xv_reverb_utt* utts_host, int64_t num_utts, const xv_reverb_noise* noises_host,
                            int64_t num_noises, int64_t wave_samples, int64_t rir_samples, int64_t noise_samples,
                            int64_t out_samples) {
  std::string err;
  const int rc = reverb_validate(utts_host, num_utts, noises_host, num_noises, wave_samples, rir_samples, noise_samples,
                                 out_samples, &err);
  if (rc != XV_OK) return fail(nullptr, rc, "xv_reverb_workspace: %s", err.c_str());
  return reverb_workspace_bytes(utts_host, num_utts, num_noises);
}

int xv_reverb(int device, const int16_t* waves_dev, int64_t wave_samples, const int16_t* rirs_dev, int64_t rir_samples,
              const int16_t* noises_dev, int64_t noise_samples, const xv_reverb_utt* utts_host, int64_t num_utts,
              const xv_reverb_noise* noises_host, int64_t num_noises, int16_t* out_i16_dev, float* out_f32_dev,
              int64_t out_samples, int32_t* status_dev, int32_t* peak_dev, int32_t* clipped_dev, void* ws_dev, int64_t ws_bytes,
              void* stream) {
  std::string err;
  const int rc = reverb_validate(utts_host, num_utts, noises_host, num_noises, wave_samples, rir_samples, noise_samples,
                                 out_samples, &err);
  if (rc != XV_OK) return fail(nullptr, rc, "xv_reverb: %s", err.c_str());
  if (!waves_dev || !status_dev || !peak_dev || !clipped_dev || (!out_i16_dev && !out_f32_dev) || (rir_samples > 0 && !rirs_dev) ||
      (noise_samples > 0 && !noises_dev))
    return fail(nullptr, XV_ERR_INVALID, "xv_reverb: null pointer");
  const int64_t need = reverb_workspace_bytes(utts_host, num_utts, num_noises);
  if (ws_bytes < need || !ws_dev)
    return fail(nullptr, XV_ERR_WORKSPACE, "xv_reverb: workspace of %lld bytes, %lld needed", (long long)(ws_dev ? ws_bytes : 0), (long long)need);
  if (reinterpret_cast<uintptr_t>(ws_dev) & 15) return fail(nullptr, XV_ERR_INVALID, "xv_reverb: the workspace must be 16-byte aligned");
  return with_device(device, "reverb", [&] {
    return launch_reverb(waves_dev, rirs_dev, noises_dev, utts_host, num_utts, noises_host, num_noises, out_i16_dev, out_f32_dev,
                         status_dev, peak_dev, clipped_dev, ws_dev, to_stream(stream));
  });
}

int64_t xv_logreg_workspace(int64_t n, int k) {
  if (k < 1 || k > XV_LOGREG_MAX_SYSTEMS) return fail(nullptr, XV_ERR_UNSUPPORTED, "xv_logreg_workspace: 1 <= k <= 8, got %d", k);
  if (n < 0 || n >= ((int64_t)1 << 40)) return fail(nullptr, XV_ERR_INVALID, "xv_logreg_workspace: n outside [0, 2^40)");
  return logreg_workspace_bytes(n, k);
}

int xv_logreg_stats(int device, const float* scores_dev, int64_t lds, int64_t n, int k, const uint8_t* targets_dev,
                    const double* theta_host, double tau, double c_tar, double c_non, const double* thresholds_host,
                    int num_thresholds, double* stats_dev, int64_t* counts_dev, void* ws_dev, int64_t ws_bytes, void* stream) {
  if (k < 1 || k > XV_LOGREG_MAX_SYSTEMS) return fail(nullptr, XV_ERR_UNSUPPORTED, "xv_logreg_stats: 1 <= k <= 8, got %d", k);
  if (n < 0 || n >= ((int64_t)1 << 40) || lds < k || !theta_host || !stats_dev || !counts_dev ||
      (n > 0 && (!scores_dev || !targets_dev)) || num_thresholds < 0 || num_thresholds > XV_LOGREG_MAX_THRESHOLDS ||
      (num_thresholds > 0 && !thresholds_host))
    return fail(nullptr, XV_ERR_INVALID, "xv_logreg_stats: bad arguments");
  const int64_t need = logreg_workspace_bytes(n, k);
  if (ws_bytes < need || (need > 0 && !ws_dev))
    return fail(nullptr, XV_ERR_WORKSPACE, "xv_logreg_stats: workspace %lld bytes < %lld", (long long)ws_bytes, (long long)need);
  if (reinterpret_cast<uintptr_t>(ws_dev) & 7) return fail(nullptr, XV_ERR_INVALID, "xv_logreg_stats: the workspace must be 8-byte aligned");
  return with_device(device, "logreg_stats", [&] {
    return launch_logreg_stats(scores_dev, lds, n, k, targets_dev, theta_host, tau, c_tar, c_non, thresholds_host,
                               num_thresholds, stats_dev, counts_dev, ws_dev, to_stream(stream));
  });
}

int xv_score_fuse(int device, const float* scores_dev, int64_t lds, int64_t n, int k, const double* theta_host, float* out_dev,
                  void* stream) {
  if (k < 1 || k > XV_LOGREG_MAX_SYSTEMS) return fail(nullptr, XV_ERR_UNSUPPORTED, "xv_score_fuse: 1 <= k <= 8, got %d", k);
  if (n < 0 || n >= ((int64_t)1 << 40) || lds < k || !theta_host || (n > 0 && (!scores_dev || !out_dev)))
    return fail(nullptr, XV_ERR_INVALID, "xv_score_fuse: bad arguments");
  return with_device(device, "score_fuse", [&] {
    return launch_score_fuse(scores_dev, lds, n, k, theta_host, out_dev, to_stream(stream));
  });
}

int xv_score_prepare(int device, const float* x_dev, int64_t ldx, int64_t n, int d_in, const float* mean_dev,
                     const float* transform_dev, int64_t ldt, int d_out, int t_cols, int normalize, float eps, float* out_dev,
                     int64_t ldo, void* stream) {
  if (!x_dev || !out_dev) return fail(nullptr, XV_ERR_INVALID, "xv_score_prepare: null pointer");
  if (n < 0 || n > INT32_MAX || d_in < 1 || d_out < 1 || ldx < d_in || ldo < d_out || !(eps >= 0.f))
    return fail(nullptr, XV_ERR_INVALID, "xv_score_prepare: bad dimensions");
  if (transform_dev) {
    if (t_cols != d_in && t_cols != d_in + 1)
      return fail(nullptr, XV_ERR_INVALID, "xv_score_prepare: a transform for %d-dimensional rows has %d or %d columns, not %d", d_in,
                  d_in, d_in + 1, t_cols);
    if (ldt < t_cols) return fail(nullptr, XV_ERR_INVALID, "xv_score_prepare: bad dimensions");
    if (out_dev == x_dev) return fail(nullptr, XV_ERR_INVALID, "xv_score_prepare: a transform cannot run in place");
    if (d_in > 2048) return fail(nullptr, XV_ERR_UNSUPPORTED, "xv_score_prepare: transforms of more than 2048 columns");
  } else if (d_out != d_in) {
    return fail(nullptr, XV_ERR_INVALID, "xv_score_prepare: d_out != d_in without a transform");
  }
  return with_device(device, "score_prepare", [&] {
    hipStream_t s = to_stream(stream);
    if (!transform_dev) return launch_score_prepare_rows(x_dev, ldx, n, d_in, mean_dev, normalize, eps, out_dev, ldo, s);
    hipError_t e = launch_score_matrix(x_dev, ldx, (int)n, transform_dev, ldt, d_out, d_in, mean_dev, t_cols == d_in + 1, out_dev, ldo, s);
    if (e == hipSuccess && normalize) e = launch_score_prepare_rows(out_dev, ldo, n, d_out, nullptr, 1, eps, out_dev, ldo, s);
    return e;
  });
}

// shared argument check of the three scoring entry points: prepared rows a [n, d], b [m, d]
static int score_operands(const char* who, const float* a, int64_t lda, int64_t n, const float* b, int64_t ldb, int64_t m, int d) {
  if (!a || !b) return fail(nullptr, XV_ERR_INVALID, "%s: null pointer", who);
  if (d < 1 || d > 2048) return fail(nullptr, XV_ERR_UNSUPPORTED, "%s: 1 <= d <= 2048, got %d", who, d);
  if (n < 0 || m < 0 || n > INT32_MAX || m > INT32_MAX || lda < d || ldb < d) return fail(nullptr, XV_ERR_INVALID, "%s: bad dimensions", who);
  return XV_OK;
}

static int check_nbins(const char* who, int nbins) {
  if (nbins < 256 || nbins > 65536 || (nbins & (nbins - 1)))
    return fail(nullptr, XV_ERR_INVALID, "%s: nbins is a power of two in 256..65536, got %d", who, nbins);
  return XV_OK;
}

int xv_score_matrix(int device, const float* a_dev, int64_t lda, int64_t n, const float* b_dev, int64_t ldb, int64_t m, int d,
                    float* out_dev, int64_t ldo, void* stream) {
  if (const int rc = score_operands("xv_score_matrix", a_dev, lda, n, b_dev, ldb, m, d)) return rc;
  if (!out_dev || ldo < m) return fail(nullptr, XV_ERR_INVALID, "xv_score_matrix: bad output");
  return with_device(device, "score_matrix", [&] {
    return launch_score_matrix(a_dev, lda, (int)n, b_dev, ldb, (int)m, d, nullptr, 0, out_dev, ldo,
                               to_stream(stream));
  });
}

int xv_score_pairs(int device, const float* a_dev, int64_t lda, int64_t n, const float* b_dev, int64_t ldb, int64_t m, int d,
                   const int32_t* ia_dev, const int32_t* ib_dev, int64_t npairs, float* out_dev, void* stream) {
  if (const int rc = score_operands("xv_score_pairs", a_dev, lda, n, b_dev, ldb, m, d)) return rc;
  if (npairs < 0 || npairs > ((int64_t)1 << 34)) return fail(nullptr, XV_ERR_INVALID, "xv_score_pairs: bad pair count");
  if (npairs > 0 && (!ia_dev || !ib_dev || !out_dev)) return fail(nullptr, XV_ERR_INVALID, "xv_score_pairs: null pointer");
  return with_device(device, "score_pairs", [&] {
    return launch_score_pairs(a_dev, lda, (int)n, b_dev, ldb, (int)m, d, ia_dev, ib_dev, npairs, out_dev,
                              to_stream(stream));
  });
}

int xv_score_histogram(int device, const float* a_dev, int64_t lda, int64_t n, const int32_t* labels_a_dev, const float* b_dev,
                       int64_t ldb, int64_t m, const int32_t* labels_b_dev, int d, int self, int nbins, uint64_t* hist_same_dev,
                       uint64_t* hist_diff_dev, void* stream) {
  if (const int rc = score_operands("xv_score_histogram", a_dev, lda, n, b_dev, ldb, m, d)) return rc;
  if (const int rc = check_nbins("xv_score_histogram", nbins)) return rc;
  if (!labels_a_dev || !labels_b_dev || !hist_same_dev || !hist_diff_dev || hist_same_dev == hist_diff_dev)
    return fail(nullptr, XV_ERR_INVALID, "xv_score_histogram: null pointer");
  if (self && (a_dev != b_dev || n != m || lda != ldb || labels_a_dev != labels_b_dev))
    return fail(nullptr, XV_ERR_INVALID, "xv_score_histogram: self needs the same rows and labels on both sides");
  return with_device(device, "score_histogram", [&] {
    return launch_score_histogram(a_dev, lda, (int)n, labels_a_dev, b_dev, ldb, (int)m, labels_b_dev, d, self ? 1 : 0, nbins,
                                  reinterpret_cast<unsigned long long*>(hist_same_dev),
                                  reinterpret_cast<unsigned long long*>(hist_diff_dev), to_stream(stream));
  });
}

// model/loss.py:133,242,328 (tf.nn.l2_normalize(w, dim=0)) and the transpose tf.layers.dense implies (:30-34)
int xv_loss_prepare_classes(int device, const float* kernel_dev, int64_t ldk, int embed_dim, int64_t num_classes, int normalize,
                            float* classes_dev, int64_t ldc, void* stream) {
  if (!kernel_dev || !classes_dev) return fail(nullptr, XV_ERR_INVALID, "xv_loss_prepare_classes: null pointer");
  if (embed_dim < 1 || embed_dim > 2048) return fail(nullptr, XV_ERR_UNSUPPORTED, "xv_loss_prepare_classes: 1 <= embed_dim <= 2048, got %d", embed_dim);
  if (num_classes < 0 || num_classes > INT32_MAX || ldk < num_classes || ldc < embed_dim)
    return fail(nullptr, XV_ERR_INVALID, "xv_loss_prepare_classes: bad dimensions");
  return with_device(device, "loss_classes", [&] {
    return launch_loss_classes(kernel_dev, ldk, embed_dim, num_classes, normalize ? 1 : 0, classes_dev, ldc,
                               to_stream(stream));
  });
}

int64_t xv_loss_workspace(int64_t n, int64_t num_classes) { return loss_workspace_bytes(n, num_classes); }

// model/loss.py:9-48 (softmax), :80-198 (asoftmax), :201-286 (additive margin), :289-384 (additive angular margin), each
// followed by tf.losses.sparse_softmax_cross_entropy; top1 = the argmax of model/trainer.py:1097
int xv_loss_classifier(int device, const float* x_dev, int64_t ldx, int64_t n, int embed_dim, const int32_t* labels_dev,
                       const float* classes_dev, int64_t ldc, int64_t num_classes, const float* bias_dev, int head, double margin,
                       double fa, float* loss_dev, float* target_dev, float* lse_dev, int32_t* top1_dev, void* ws_dev,
                       int64_t ws_bytes, void* stream) {
  if (!x_dev || !labels_dev || !classes_dev || !loss_dev || !target_dev || !lse_dev || !top1_dev || !ws_dev)
    return fail(nullptr, XV_ERR_INVALID, "xv_loss_classifier: null pointer");
  if (embed_dim < 1 || embed_dim > 2048) return fail(nullptr, XV_ERR_UNSUPPORTED, "xv_loss_classifier: 1 <= embed_dim <= 2048, got %d", embed_dim);
  if (n < 0 || n > INT32_MAX || num_classes < 1 || num_classes > INT32_MAX || ldx < embed_dim || ldc < embed_dim)
    return fail(nullptr, XV_ERR_INVALID, "xv_loss_classifier: bad dimensions");
  if (head < XV_LOSS_SOFTMAX || head > XV_LOSS_ARCSOFTMAX) return fail(nullptr, XV_ERR_INVALID, "xv_loss_classifier: unknown head %d", head);
  if (bias_dev && head != XV_LOSS_SOFTMAX) return fail(nullptr, XV_ERR_INVALID, "xv_loss_classifier: only the softmax head has a bias");
  int m = 0;
  if (head == XV_LOSS_ASOFTMAX) {
    if (margin != 1.0 && margin != 2.0 && margin != 4.0)
      return fail(nullptr, XV_ERR_UNSUPPORTED, "xv_loss_classifier: m=%g is not supported (asoftmax: 1, 2 or 4)", margin);   // loss.py:168
    m = (int)margin;
  }
  if (!(fa >= 0.0 && fa <= 1.0) || !std::isfinite(margin)) return fail(nullptr, XV_ERR_INVALID, "xv_loss_classifier: bad margin or fa");
  if (ws_bytes < loss_workspace_bytes(n, num_classes))
    return fail(nullptr, XV_ERR_WORKSPACE, "xv_loss_classifier: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
                (long long)loss_workspace_bytes(n, num_classes));
  if (n == 0) return XV_OK;
  DeviceGuard g(device);
  if (!g.ok) return fail(nullptr, XV_ERR_HIP, "cannot select HIP device %d", device);
  hipStream_t s = to_stream(stream);
  hipError_t e = launch_loss_rows(x_dev, ldx, n, embed_dim, labels_dev, classes_dev, ldc, num_classes, bias_dev, head, m, margin, fa,
                                  target_dev, ws_dev, s);
  int bad = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&bad, ws_dev, sizeof(int), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail(nullptr, XV_ERR_HIP, "loss_rows failed: %s", hipGetErrorString(e));
  if (bad) return fail(nullptr, XV_ERR_INVALID, "xv_loss_classifier: a label lies outside [0, %lld)", (long long)num_classes);
  e = launch_loss_tiles(x_dev, ldx, (int)n, embed_dim, labels_dev, classes_dev, ldc, (int)num_classes, bias_dev, target_dev,
                        loss_dev, lse_dev, top1_dev, ws_dev, s);
  if (e != hipSuccess) return fail(nullptr, XV_ERR_HIP, "loss_tiles launch failed: %s", hipGetErrorString(e));
  return XV_OK;
}

int64_t xv_loss_grad_workspace(int64_t n, int64_t num_classes, int embed_dim) {
  return loss_grad_workspace_bytes(n, num_classes, embed_dim, 0);
}

int64_t xv_loss_grad_workspace_min(int64_t n, int64_t num_classes, int embed_dim) {
  return loss_grad_workspace_bytes(n, num_classes, embed_dim, 1);
}

// xv_loss_classifier and TensorFlow's gradients of it with respect to x, the raw kernel and the bias (include/xvec_hip.h)
int xv_loss_classifier_grad(int device, const float* x_dev, int64_t ldx, int64_t n, int embed_dim, const int32_t* labels_dev,
                            const float* rows_dev, int64_t ldc, int64_t num_classes, const float* bias_dev, int head, double margin,
                            double fa, double grad_scale, float* loss_dev, float* target_dev, float* lse_dev, int32_t* top1_dev,
                            float* grad_x_dev, int64_t ldgx, float* grad_rows_dev, float* grad_bias_dev, void* ws_dev,
                            int64_t ws_bytes, void* stream) {
  if (!x_dev || !labels_dev || !rows_dev || !loss_dev || !target_dev || !lse_dev || !top1_dev || !grad_rows_dev || !ws_dev)
    return fail(nullptr, XV_ERR_INVALID, "xv_loss_classifier_grad: null pointer");
  if (embed_dim < 1 || embed_dim > 2048)
    return fail(nullptr, XV_ERR_UNSUPPORTED, "xv_loss_classifier_grad: 1 <= embed_dim <= 2048, got %d", embed_dim);
  if (n < 0 || n > INT32_MAX || num_classes < 1 || num_classes > INT32_MAX || ldx < embed_dim || ldc < embed_dim ||
      (grad_x_dev && ldgx < embed_dim))
    return fail(nullptr, XV_ERR_INVALID, "xv_loss_classifier_grad: bad dimensions");
  if (head < XV_LOSS_SOFTMAX || head > XV_LOSS_ARCSOFTMAX) return fail(nullptr, XV_ERR_INVALID, "xv_loss_classifier_grad: unknown head %d", head);
  if (bias_dev && head != XV_LOSS_SOFTMAX) return fail(nullptr, XV_ERR_INVALID, "xv_loss_classifier_grad: only the softmax head has a bias");
  if (bias_dev && !grad_bias_dev) return fail(nullptr, XV_ERR_INVALID, "xv_loss_classifier_grad: a bias needs grad_bias_dev");
  int m = 0;
  if (head == XV_LOSS_ASOFTMAX) {
    if (margin != 1.0 && margin != 2.0 && margin != 4.0)
      return fail(nullptr, XV_ERR_UNSUPPORTED, "xv_loss_classifier_grad: m=%g is not supported (asoftmax: 1, 2 or 4)", margin);   // loss.py:168
    m = (int)margin;
  }
  if (!(fa >= 0.0 && fa <= 1.0) || !std::isfinite(margin) || !std::isfinite(grad_scale))
    return fail(nullptr, XV_ERR_INVALID, "xv_loss_classifier_grad: bad margin, fa or grad_scale");
  if ((reinterpret_cast<uintptr_t>(ws_dev) & 15) != 0)
    return fail(nullptr, XV_ERR_INVALID, "xv_loss_classifier_grad: the workspace must be 16-byte aligned");
  const int64_t need = loss_grad_workspace_bytes(n, num_classes, embed_dim, 1);
  if (ws_bytes < need)
    return fail(nullptr, XV_ERR_WORKSPACE, "xv_loss_classifier_grad: workspace of %lld bytes, at least %lld needed", (long long)ws_bytes,
                (long long)need);
  if (n == 0) return XV_OK;
  DeviceGuard g(device);
  if (!g.ok) return fail(nullptr, XV_ERR_HIP, "cannot select HIP device %d", device);
  hipStream_t s = to_stream(stream);
  hipError_t e = launch_loss_grad_forward_rows(x_dev, ldx, n, embed_dim, labels_dev, rows_dev, ldc, num_classes, bias_dev, head, m,
                                               margin, fa, ws_dev, s);
  int bad = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&bad, ws_dev, sizeof(int), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail(nullptr, XV_ERR_HIP, "loss_grad rows failed: %s", hipGetErrorString(e));
  if (bad) return fail(nullptr, XV_ERR_INVALID, "xv_loss_classifier_grad: a label lies outside [0, %lld)", (long long)num_classes);
  e = launch_loss_grad_rest(x_dev, ldx, (int)n, embed_dim, labels_dev, rows_dev, ldc, (int)num_classes, bias_dev, head, m, margin, fa,
                            grad_scale, loss_dev, target_dev, lse_dev, top1_dev, grad_x_dev, ldgx, grad_rows_dev,
                            bias_dev ? grad_bias_dev : nullptr, ws_dev, ws_bytes, s);
  if (e != hipSuccess) return fail(nullptr, XV_ERR_HIP, "loss_grad launch failed: %s", hipGetErrorString(e));
  return XV_OK;
}

int64_t xv_opt_workspace(int64_t count) { return opt_workspace_bytes(count); }

// model/trainer.py:225-246, 529-533 and model/loss.py:26-33: l2, tf.clip_by_norm, then sgd / momentum / adam
int xv_opt_step(int device, int kind, int use_nesterov, float* w_dev, const float* grad_dev, float* slot0_dev, float* slot1_dev,
                int64_t count, double learning_rate, double l2, double clip_norm, double momentum, int64_t step, void* ws_dev,
                int64_t ws_bytes, void* stream) {
  if (kind < XV_OPT_SGD || kind > XV_OPT_ADAM) return fail(nullptr, XV_ERR_INVALID, "xv_opt_step: unknown kind %d", kind);
  if (count < 0) return fail(nullptr, XV_ERR_INVALID, "xv_opt_step: count = %lld", (long long)count);
  if (!std::isfinite(learning_rate) || learning_rate < 0.0) return fail(nullptr, XV_ERR_INVALID, "xv_opt_step: learning_rate must be finite and >= 0");
  if (!(l2 >= 0.0) || !std::isfinite(l2) || !(clip_norm >= 0.0) || !std::isfinite(clip_norm))
    return fail(nullptr, XV_ERR_INVALID, "xv_opt_step: l2 and clip_norm must be finite and >= 0");
  if (kind == XV_OPT_MOMENTUM && (!std::isfinite(momentum) || momentum < 0.0)) return fail(nullptr, XV_ERR_INVALID, "xv_opt_step: bad momentum");
  if (kind == XV_OPT_ADAM && step < 1) return fail(nullptr, XV_ERR_INVALID, "xv_opt_step: adam counts its steps from 1, got %lld", (long long)step);
  if (count == 0) return XV_OK;
  if (!w_dev || !grad_dev || (kind != XV_OPT_SGD && !slot0_dev) || (kind == XV_OPT_ADAM && !slot1_dev))
    return fail(nullptr, XV_ERR_INVALID, "xv_opt_step: null pointer");
  if ((float)clip_norm > 0.f) {
    if (!ws_dev || ws_bytes < opt_workspace_bytes(count))
      return fail(nullptr, XV_ERR_WORKSPACE, "xv_opt_step: workspace of %lld bytes, %lld needed", (long long)(ws_dev ? ws_bytes : 0),
                  (long long)opt_workspace_bytes(count));
    if ((reinterpret_cast<uintptr_t>(ws_dev) & 7) != 0) return fail(nullptr, XV_ERR_INVALID, "xv_opt_step: the workspace must be 8-byte aligned");
  }
  return with_device(device, "xv_opt_step", [&] {
    return launch_opt_step(kind, use_nesterov ? 1 : 0, w_dev, grad_dev, slot0_dev, slot1_dev, count, learning_rate, l2, clip_norm,
                           momentum, step, ws_dev, to_stream(stream));
  });
}

int64_t xv_seg_workspace(int64_t n, int in_dim, int out_dim) { return seg_workspace_bytes(n, in_dim, out_dim, 0); }

int64_t xv_seg_workspace_min(int64_t n, int in_dim, int out_dim) { return seg_workspace_bytes(n, in_dim, out_dim, 1); }

namespace {

// what every trained layer's calls check of the batch-norm pointers (all four or none) and the activation; `op` names the caller
int layer_lines_check(const char* op, const void* gamma, const void* beta, const void* mm, const void* mv, int act) {
  const int given = (gamma != nullptr) + (beta != nullptr) + (mm != nullptr) + (mv != nullptr);
  if (given != 0 && given != 4)
    return fail(nullptr, XV_ERR_INVALID, "%s: batch norm needs gamma, beta, moving_mean and moving_variance, or none of them", op);
  if (act < XV_SEG_ACT_NONE || act > XV_SEG_ACT_LRELU) return fail(nullptr, XV_ERR_INVALID, "%s: unknown activation %d", op, act);
  return XV_OK;
}

// the workspace of a trained layer's call: `need` bytes at a 16-byte aligned address
int layer_ws_check(const char* op, const void* ws_dev, int64_t ws_bytes, int64_t need) {
  if (!ws_dev || ws_bytes < need)
    return fail(nullptr, XV_ERR_WORKSPACE, "%s: workspace of %lld bytes, at least %lld needed", op, (long long)(ws_dev ? ws_bytes : 0),
                (long long)need);
  if ((reinterpret_cast<uintptr_t>(ws_dev) & 15) != 0)
    return fail(nullptr, XV_ERR_INVALID, "%s: the workspace must be 16-byte aligned", op);
  return XV_OK;
}

// the checks the two calls of a segment-level layer share; `op` names the caller in the message
int seg_check(const char* op, int64_t n, int in_dim, int out_dim, int64_t ldx, int64_t ldw, const void* gamma, const void* beta,
              const void* mm, const void* mv, int act) {
  if (in_dim < 1 || in_dim > 16384 || out_dim < 1 || out_dim > 4096 || n > (1 << 24))
    return fail(nullptr, XV_ERR_UNSUPPORTED, "%s: 1 <= in_dim <= 16384, 1 <= out_dim <= 4096, n <= 2^24, got %d, %d, %lld", op, in_dim,
                out_dim, (long long)n);
  if (n < 0 || ldx < in_dim || ldw < in_dim) return fail(nullptr, XV_ERR_INVALID, "%s: bad dimensions", op);
  return layer_lines_check(op, gamma, beta, mm, mv, act);
}

}  // namespace

// dense + inference-mode batch norm + activation with the current weights (include/xvec_hip.h)
int xv_seg_forward(int device, const float* x_dev, int64_t ldx, int64_t n, int in_dim, const float* w_dev, int64_t ldw, int out_dim,
                   const float* bias_dev, const float* gamma_dev, const float* beta_dev, const float* mean_dev, const float* var_dev,
                   int act, float* z_dev, int64_t ldz, float* y_dev, int64_t ldy, void* stream) {
  if (!x_dev || !w_dev || !bias_dev || !z_dev || !y_dev) return fail(nullptr, XV_ERR_INVALID, "xv_seg_forward: null pointer");
  const int rc = seg_check("xv_seg_forward", n, in_dim, out_dim, ldx, ldw, gamma_dev, beta_dev, mean_dev, var_dev, act);
  if (rc != XV_OK) return rc;
  if (ldz < out_dim || ldy < out_dim) return fail(nullptr, XV_ERR_INVALID, "xv_seg_forward: bad dimensions");
  if (n == 0) return XV_OK;
  return with_device(device, "xv_seg_forward", [&] {
    return launch_seg_forward(x_dev, ldx, (int)n, in_dim, w_dev, ldw, out_dim, bias_dev, gamma_dev, beta_dev, mean_dev, var_dev, act,
                              z_dev, ldz, y_dev, ldy, to_stream(stream));
  });
}

int xv_seg_backward(int device, const float* gy_dev, int64_t ldgy, const float* x_dev, int64_t ldx, const float* z_dev, int64_t ldz,
                    int64_t n, int in_dim, const float* w_dev, int64_t ldw, int out_dim, const float* gamma_dev,
                    const float* beta_dev, const float* mean_dev, const float* var_dev, int act, float* gx_dev, int64_t ldgx,
                    float* gw_dev, float* gbias_dev, float* ggamma_dev, float* gbeta_dev, void* ws_dev, int64_t ws_bytes,
                    void* stream) {
  if (!gy_dev || !x_dev || !z_dev || !w_dev || !gw_dev || !gbias_dev)
    return fail(nullptr, XV_ERR_INVALID, "xv_seg_backward: null pointer");
  int rc = seg_check("xv_seg_backward", n, in_dim, out_dim, ldx, ldw, gamma_dev, beta_dev, mean_dev, var_dev, act);
  if (rc != XV_OK) return rc;
  if (gamma_dev && (!ggamma_dev || !gbeta_dev))
    return fail(nullptr, XV_ERR_INVALID, "xv_seg_backward: batch norm needs ggamma_dev and gbeta_dev");
  if (ldgy < out_dim || ldz < out_dim || (gx_dev && ldgx < in_dim)) return fail(nullptr, XV_ERR_INVALID, "xv_seg_backward: bad dimensions");
  if (n == 0) return XV_OK;
  if ((rc = layer_ws_check("xv_seg_backward", ws_dev, ws_bytes, seg_workspace_bytes(n, in_dim, out_dim, 1))) != XV_OK) return rc;
  return with_device(device, "xv_seg_backward", [&] {
    return launch_seg_backward(gy_dev, ldgy, x_dev, ldx, z_dev, ldz, (int)n, in_dim, w_dev, ldw, out_dim, gamma_dev, beta_dev, mean_dev,
                               var_dev, act, gx_dev, ldgx, gw_dev, gbias_dev, ggamma_dev, gbeta_dev, ws_dev, ws_bytes,
                               to_stream(stream));
  });
}

namespace {

// the checks the two statistics-pooling calls share; `op` names the caller in the message
int stat_pool_check(const char* op, int channels, int64_t batch, int64_t total_rows, int64_t ldx, int64_t ldp, int64_t ldv) {
  if (channels < 1 || channels > 4096 || total_rows > (1 << 24))
    return fail(nullptr, XV_ERR_UNSUPPORTED, "%s: 1 <= channels <= 4096, total_rows <= 2^24, got %d, %lld", op, channels,
                (long long)total_rows);
  if (batch < 0 || total_rows < 0 || ldx < channels || ldp < 2 * (int64_t)channels || ldv < channels)
    return fail(nullptr, XV_ERR_INVALID, "%s: bad dimensions", op);
  return XV_OK;
}

}  // namespace

// statistics pooling of the caller's packed rows, and its gradient (include/xvec_hip.h, csrc/pool_grad.hip)
int xv_stat_pool_forward(int device, const float* x_dev, int64_t ldx, int channels, const int32_t* offsets_dev, int64_t batch,
                         int64_t total_rows, float* pooled_dev, int64_t ldp, float* var_dev, int64_t ldv, void* stream) {
  const int rc = stat_pool_check("xv_stat_pool_forward", channels, batch, total_rows, ldx, ldp, ldv);
  if (rc != XV_OK) return rc;
  if (batch == 0) return XV_OK;
  if (!x_dev || !offsets_dev || !pooled_dev || !var_dev) return fail(nullptr, XV_ERR_INVALID, "xv_stat_pool_forward: null pointer");
  if (batch > (int64_t)1 << 24) return fail(nullptr, XV_ERR_UNSUPPORTED, "xv_stat_pool_forward: batch <= 2^24, got %lld", (long long)batch);
  return with_device(device, "xv_stat_pool_forward", [&] {
    return launch_stat_pool_forward(x_dev, ldx, channels, offsets_dev, batch, total_rows, pooled_dev, ldp, var_dev, ldv,
                                    to_stream(stream));
  });
}

int xv_stat_pool_backward(int device, const float* gp_dev, int64_t ldgp, const float* x_dev, int64_t ldx, int channels,
                          const int32_t* offsets_dev, int64_t batch, int64_t total_rows, const float* pooled_dev, int64_t ldp,
                          const float* var_dev, int64_t ldv, float* gx_dev, int64_t ldgx, void* stream) {
  const int rc = stat_pool_check("xv_stat_pool_backward", channels, batch, total_rows, ldx, ldp, ldv);
  if (rc != XV_OK) return rc;
  if (ldgp < 2 * (int64_t)channels || ldgx < channels) return fail(nullptr, XV_ERR_INVALID, "xv_stat_pool_backward: bad dimensions");
  if (batch == 0) return XV_OK;
  if (!gp_dev || !x_dev || !offsets_dev || !pooled_dev || !var_dev || !gx_dev)
    return fail(nullptr, XV_ERR_INVALID, "xv_stat_pool_backward: null pointer");
  if (batch > (int64_t)1 << 24) return fail(nullptr, XV_ERR_UNSUPPORTED, "xv_stat_pool_backward: batch <= 2^24, got %lld", (long long)batch);
  return with_device(device, "xv_stat_pool_backward", [&] {
    return launch_stat_pool_backward(gp_dev, ldgp, x_dev, ldx, channels, offsets_dev, batch, total_rows, pooled_dev, ldp, var_dev,
                                     ldv, gx_dev, ldgx, to_stream(stream));
  });
}

namespace {

// the shapes of one attentive-pooling call: per-head widths and the pooled width, or the status that refuses them
struct AttShape { int dq, dv, P; };

int att_pool_check(const char* op, int heads, int key_dim, int value_dim, int split_key, int split_value, int64_t batch,
                   int64_t total_rows, int64_t ldk, int64_t ldv, int64_t ldq, int64_t ldw, int64_t ldp, int64_t ldvar, AttShape* sh) {
  if (heads < 1 || heads > 16 || key_dim < 1 || key_dim > 4096 || value_dim < 1 || value_dim > 4096 || total_rows > (1 << 24) ||
      batch > (1 << 20))
    return fail(nullptr, XV_ERR_UNSUPPORTED,
                "%s: 1 <= heads <= 16, 1 <= key_dim, value_dim <= 4096, total_rows <= 2^24, batch <= 2^20, got %d, %d, %d, %lld, %lld",
                op, heads, key_dim, value_dim, (long long)total_rows, (long long)batch);
  if ((split_key && key_dim % heads != 0) || (split_value && value_dim % heads != 0))
    return fail(nullptr, XV_ERR_INVALID, "%s: a split dimension must be a multiple of heads", op);
  sh->dq = split_key ? key_dim / heads : key_dim;
  sh->dv = split_value ? value_dim / heads : value_dim;
  sh->P = heads * sh->dv;
  if (batch < 0 || total_rows < 0 || ldk < key_dim || ldv < value_dim || ldq < sh->dq || ldw < heads || ldp < 2 * (int64_t)sh->P ||
      ldvar < sh->P)
    return fail(nullptr, XV_ERR_INVALID, "%s: bad dimensions", op);
  return XV_OK;
}

int64_t att_pool_ws(int64_t batch, int64_t total_rows, int heads, int key_dim, int value_dim, int split_key, int split_value,
                    bool least) {
  AttShape sh;
  const int rc = att_pool_check("xv_att_pool_workspace", heads, key_dim, value_dim, split_key, split_value, batch, total_rows, key_dim,
                                value_dim, key_dim, heads, (int64_t)1 << 40, (int64_t)1 << 40, &sh);
  if (rc != XV_OK) return rc;
  return att_pool_workspace_bytes(batch, total_rows, heads, sh.dq, sh.P, least ? 1 : batch);
}

}  // namespace

// self-attentive pooling of the caller's packed rows, and its gradient (include/xvec_hip.h, csrc/att_pool_grad.hip)
int64_t xv_att_pool_workspace(int64_t batch, int64_t total_rows, int heads, int key_dim, int value_dim, int split_key,
                              int split_value) {
  return att_pool_ws(batch, total_rows, heads, key_dim, value_dim, split_key, split_value, false);
}

int64_t xv_att_pool_workspace_min(int64_t batch, int64_t total_rows, int heads, int key_dim, int value_dim, int split_key,
                                  int split_value) {
  return att_pool_ws(batch, total_rows, heads, key_dim, value_dim, split_key, split_value, true);
}

int xv_att_pool_forward(int device, const float* key_dev, int64_t ldk, int key_dim, const float* value_dev, int64_t ldv, int value_dim,
                        const float* query_dev, int64_t ldq, int heads, int split_key, int split_value, float scale,
                        const int32_t* offsets_dev, int64_t batch, int64_t total_rows, float* weights_dev, int64_t ldw,
                        float* pooled_dev, int64_t ldp, float* var_dev, int64_t ldvar, void* stream) {
  AttShape sh;
  const int rc = att_pool_check("xv_att_pool_forward", heads, key_dim, value_dim, split_key, split_value, batch, total_rows, ldk, ldv,
                                ldq, ldw, ldp, ldvar, &sh);
  if (rc != XV_OK) return rc;
  if (batch == 0) return XV_OK;
  if (!key_dev || !value_dev || !query_dev || !offsets_dev || !weights_dev || !pooled_dev || !var_dev)
    return fail(nullptr, XV_ERR_INVALID, "xv_att_pool_forward: null pointer");
  return with_device(device, "xv_att_pool_forward", [&] {
    return launch_att_pool_forward(key_dev, ldk, sh.dq, split_key != 0, value_dev, ldv, sh.dv, split_value != 0, query_dev, ldq, heads,
                                   scale, offsets_dev, batch, total_rows, weights_dev, ldw, pooled_dev, ldp, var_dev, ldvar,
                                   to_stream(stream));
  });
}

int xv_att_pool_backward(int device, const float* gp_dev, int64_t ldgp, const float* key_dev, int64_t ldk, int key_dim,
                         const float* value_dev, int64_t ldv, int value_dim, const float* query_dev, int64_t ldq, int heads,
                         int split_key, int split_value, float scale, const int32_t* offsets_dev, int64_t batch, int64_t total_rows,
                         const float* weights_dev, int64_t ldw, const float* pooled_dev, int64_t ldp, const float* var_dev,
                         int64_t ldvar, float* gkey_dev, int64_t ldgk, float* gvalue_dev, int64_t ldgv, float* gquery_dev,
                         int64_t ldgq, void* ws_dev, int64_t ws_bytes, void* stream) {
  AttShape sh;
  int rc = att_pool_check("xv_att_pool_backward", heads, key_dim, value_dim, split_key, split_value, batch, total_rows, ldk, ldv, ldq,
                          ldw, ldp, ldvar, &sh);
  if (rc != XV_OK) return rc;
  if (ldgp < 2 * (int64_t)sh.P || ldgk < key_dim || ldgv < value_dim || ldgq < sh.dq)
    return fail(nullptr, XV_ERR_INVALID, "xv_att_pool_backward: bad dimensions");
  if (batch == 0) return XV_OK;
  if (!gp_dev || !key_dev || !value_dev || !query_dev || !offsets_dev || !weights_dev || !pooled_dev || !var_dev || !gkey_dev ||
      !gvalue_dev || !gquery_dev)
    return fail(nullptr, XV_ERR_INVALID, "xv_att_pool_backward: null pointer");
  if ((rc = layer_ws_check("xv_att_pool_backward", ws_dev, ws_bytes,
                           att_pool_workspace_bytes(batch, total_rows, heads, sh.dq, sh.P, 1))) != XV_OK)
    return rc;
  return with_device(device, "xv_att_pool_backward", [&] {
    return launch_att_pool_backward(gp_dev, ldgp, key_dev, ldk, sh.dq, split_key != 0, value_dev, ldv, sh.dv, split_value != 0,
                                    query_dev, ldq, heads, scale, offsets_dev, batch, total_rows, weights_dev, ldw, pooled_dev, ldp,
                                    var_dev, ldvar, gkey_dev, ldgk, gvalue_dev, ldgv, gquery_dev, ldgq, ws_dev, ws_bytes,
                                    to_stream(stream));
  });
}

// a frame-level layer on packed utterances: W-tap temporal convolution + batch norm + activation (include/xvec_hip.h,
// csrc/tconv_grad.hip)
int64_t xv_tconv_workspace(int64_t batch, int64_t total_in, int64_t total_out, int taps, int channels, int out_dim) {
  return tconv_workspace_bytes(batch, total_in, total_out, taps, channels, out_dim);
}

int64_t xv_tconv_workspace_min(int64_t batch, int64_t total_in, int64_t total_out, int taps, int channels, int out_dim) {
  return tconv_workspace_bytes(batch, total_in, total_out, taps, channels, out_dim);
}

int64_t xv_tconv_forward_workspace(int64_t batch, int64_t total_out) { return tconv_forward_workspace_bytes(batch, total_out); }

namespace {

// the checks the two calls of a temporal-convolution layer share; `op` names the caller in the message
int tconv_check(const char* op, int taps, int channels, int out_dim, int64_t batch, int64_t total_in, int64_t total_out, int64_t ldx,
                int64_t ldw, const void* gamma, const void* beta, const void* mm, const void* mv, int act) {
  if (taps < 1 || taps > 16 || channels < 1 || (int64_t)taps * channels > 16384 || out_dim < 1 || out_dim > 4096 ||
      batch > (1 << 24) || total_in > (1 << 24) || total_out > (1 << 24))
    return fail(nullptr, XV_ERR_UNSUPPORTED,
                "%s: 1 <= taps <= 16, taps * channels <= 16384, 1 <= out_dim <= 4096, batch and rows <= 2^24, got %d, %d, %d, %lld, "
                "%lld, %lld", op, taps, channels, out_dim, (long long)batch, (long long)total_in, (long long)total_out);
  if (batch < 0 || total_in < 0 || total_out < 0 || ldx < channels || ldw < (int64_t)taps * channels)
    return fail(nullptr, XV_ERR_INVALID, "%s: bad dimensions", op);
  return layer_lines_check(op, gamma, beta, mm, mv, act);
}

}  // namespace

int xv_tconv_forward(int device, const float* x_dev, int64_t ldx, int channels, int taps, const int32_t* offsets_dev, int64_t batch,
                     int64_t total_in, int64_t total_out, const float* w_dev, int64_t ldw, int out_dim, const float* bias_dev,
                     const float* gamma_dev, const float* beta_dev, const float* mean_dev, const float* var_dev, int act,
                     float* z_dev, int64_t ldz, float* y_dev, int64_t ldy, void* ws_dev, int64_t ws_bytes, void* stream) {
  if (!x_dev || !offsets_dev || !w_dev || !bias_dev || !z_dev || !y_dev)
    return fail(nullptr, XV_ERR_INVALID, "xv_tconv_forward: null pointer");
  int rc = tconv_check("xv_tconv_forward", taps, channels, out_dim, batch, total_in, total_out, ldx, ldw, gamma_dev, beta_dev, mean_dev,
                       var_dev, act);
  if (rc != XV_OK) return rc;
  if (ldz < out_dim || ldy < out_dim) return fail(nullptr, XV_ERR_INVALID, "xv_tconv_forward: bad dimensions");
  if (batch == 0 || total_out == 0) return XV_OK;
  if ((rc = layer_ws_check("xv_tconv_forward", ws_dev, ws_bytes, tconv_forward_workspace_bytes(batch, total_out))) != XV_OK) return rc;
  return with_device(device, "xv_tconv_forward", [&] {
    return launch_tconv_forward(x_dev, ldx, channels, taps, offsets_dev, batch, total_in, total_out, w_dev, ldw, out_dim, bias_dev,
                                gamma_dev, beta_dev, mean_dev, var_dev, act, z_dev, ldz, y_dev, ldy, ws_dev, to_stream(stream));
  });
}

int xv_tconv_backward(int device, const float* gy_dev, int64_t ldgy, const float* x_dev, int64_t ldx, int channels, int taps,
                      const int32_t* offsets_dev, int64_t batch, int64_t total_in, int64_t total_out, const float* z_dev, int64_t ldz,
                      const float* w_dev, int64_t ldw, int out_dim, const float* gamma_dev, const float* beta_dev,
                      const float* mean_dev, const float* var_dev, int act, float* gx_dev, int64_t ldgx, float* gw_dev,
                      float* gbias_dev, float* ggamma_dev, float* gbeta_dev, void* ws_dev, int64_t ws_bytes, void* stream) {
  if (!gy_dev || !x_dev || !offsets_dev || !z_dev || !w_dev || !gw_dev || !gbias_dev)
    return fail(nullptr, XV_ERR_INVALID, "xv_tconv_backward: null pointer");
  int rc = tconv_check("xv_tconv_backward", taps, channels, out_dim, batch, total_in, total_out, ldx, ldw, gamma_dev, beta_dev,
                       mean_dev, var_dev, act);
  if (rc != XV_OK) return rc;
  if (gamma_dev && (!ggamma_dev || !gbeta_dev))
    return fail(nullptr, XV_ERR_INVALID, "xv_tconv_backward: batch norm needs ggamma_dev and gbeta_dev");
  if (ldgy < out_dim || ldz < out_dim || (gx_dev && ldgx < channels))
    return fail(nullptr, XV_ERR_INVALID, "xv_tconv_backward: bad dimensions");
  if (batch == 0 || total_out == 0) return XV_OK;
  if (total_in < total_out) return fail(nullptr, XV_ERR_INVALID, "xv_tconv_backward: total_in below total_out");
  if ((rc = layer_ws_check("xv_tconv_backward", ws_dev, ws_bytes,
                           tconv_workspace_bytes(batch, total_in, total_out, taps, channels, out_dim))) != XV_OK)
    return rc;
  return with_device(device, "xv_tconv_backward", [&] {
    return launch_tconv_backward(gy_dev, ldgy, x_dev, ldx, channels, taps, offsets_dev, batch, total_in, total_out, z_dev, ldz, w_dev,
                                 ldw, out_dim, gamma_dev, beta_dev, mean_dev, var_dev, act, gx_dev, ldgx, gw_dev, gbias_dev,
                                 ggamma_dev, gbeta_dev, ws_dev, to_stream(stream));
  });
}

namespace {

bool gconv_window_ok(int kh, int kw, int st, int sf) {
  return (kh == 1 || kh == 3) && (kw == 1 || kw == 3) && (st == 1 || st == 2) && (sf == 1 || sf == 2);
}

// the checks the two calls of a grid convolution share; `op` names the caller in the message
int gconv_check(const char* op, int channels, int bins, int kh, int kw, int st, int sf, int out_dim, int64_t batch, int64_t total_in,
                int64_t total_out, int64_t ldx, int64_t ldw, const void* gamma, const void* beta, const void* mm, const void* mv,
                int act) {
  if (!gconv_window_ok(kh, kw, st, sf))
    return fail(nullptr, XV_ERR_UNSUPPORTED, "%s: kh, kw in {1, 3} and st, sf in {1, 2}, got %d, %d, %d, %d", op, kh, kw, st, sf);
  if (channels < 1 || (int64_t)kh * kw * channels > 16384 || out_dim < 1 || out_dim > 4096 || bins < 1 || bins > 4096 ||
      batch > (1 << 24) || total_in > (1 << 24) || total_out > (1 << 24) || total_in * bins > (1 << 24) ||
      total_out * ((bins + sf - 1) / sf) > (1 << 24))
    return fail(nullptr, XV_ERR_UNSUPPORTED,
                "%s: kh * kw * channels <= 16384, 1 <= out_dim, bins <= 4096, batch and rows <= 2^24, got %d, %d, %d, %lld, %lld, %lld",
                op, channels, out_dim, bins, (long long)batch, (long long)total_in, (long long)total_out);
  if (batch < 0 || total_in < 0 || total_out < 0 || ldx < channels || ldw < (int64_t)kh * kw * channels)
    return fail(nullptr, XV_ERR_INVALID, "%s: bad dimensions", op);
  return layer_lines_check(op, gamma, beta, mm, mv, act);
}

}  // namespace

// a grid convolution of the ResNet on packed utterances + batch norm + activation, and the residual join (include/xvec_hip.h,
// csrc/gconv_grad.hip)
int64_t xv_gconv_workspace(int64_t batch, int64_t total_in, int64_t total_out, int bins, int kh, int kw, int st, int sf, int channels,
                           int out_dim) {
  if (!gconv_window_ok(kh, kw, st, sf)) return XV_ERR_UNSUPPORTED;
  return gconv_workspace_bytes(batch, total_in, total_out, bins, kh, kw, st, sf, channels, out_dim);
}

int64_t xv_gconv_workspace_min(int64_t batch, int64_t total_in, int64_t total_out, int bins, int kh, int kw, int st, int sf,
                               int channels, int out_dim) {
  return xv_gconv_workspace(batch, total_in, total_out, bins, kh, kw, st, sf, channels, out_dim);
}

int64_t xv_gconv_forward_workspace(int64_t batch, int64_t total_out, int bins, int sf) {
  if (sf != 1 && sf != 2) return XV_ERR_UNSUPPORTED;
  return gconv_forward_workspace_bytes(batch, total_out, bins, sf);
}

int xv_gconv_forward(int device, const float* x_dev, int64_t ldx, int channels, int bins, int kh, int kw, int st, int sf,
                     const int32_t* offsets_dev, int64_t batch, int64_t total_in, int64_t total_out, const float* w_dev, int64_t ldw,
                     int out_dim, const float* bias_dev, const float* gamma_dev, const float* beta_dev, const float* mean_dev,
                     const float* var_dev, int act, float* z_dev, int64_t ldz, float* y_dev, int64_t ldy, void* ws_dev,
                     int64_t ws_bytes, void* stream) {
  if (!x_dev || !offsets_dev || !w_dev || !z_dev || !y_dev) return fail(nullptr, XV_ERR_INVALID, "xv_gconv_forward: null pointer");
  int rc = gconv_check("xv_gconv_forward", channels, bins, kh, kw, st, sf, out_dim, batch, total_in, total_out, ldx, ldw, gamma_dev,
                       beta_dev, mean_dev, var_dev, act);
  if (rc != XV_OK) return rc;
  if (ldz < out_dim || ldy < out_dim) return fail(nullptr, XV_ERR_INVALID, "xv_gconv_forward: bad dimensions");
  if (batch == 0 || total_out == 0) return XV_OK;
  if ((rc = layer_ws_check("xv_gconv_forward", ws_dev, ws_bytes, gconv_forward_workspace_bytes(batch, total_out, bins, sf))) != XV_OK)
    return rc;
  return with_device(device, "xv_gconv_forward", [&] {
    return launch_gconv_forward(x_dev, ldx, channels, bins, kh, kw, st, sf, offsets_dev, batch, total_in, total_out, w_dev, ldw,
                                out_dim, bias_dev, gamma_dev, beta_dev, mean_dev, var_dev, act, z_dev, ldz, y_dev, ldy, ws_dev,
                                to_stream(stream));
  });
}

int xv_gconv_backward(int device, const float* gy_dev, int64_t ldgy, const float* x_dev, int64_t ldx, int channels, int bins, int kh,
                      int kw, int st, int sf, const int32_t* offsets_dev, int64_t batch, int64_t total_in, int64_t total_out,
                      const float* z_dev, int64_t ldz, const float* w_dev, int64_t ldw, int out_dim, const float* gamma_dev,
                      const float* beta_dev, const float* mean_dev, const float* var_dev, int act, float* gx_dev, int64_t ldgx,
                      float* gw_dev, float* gbias_dev, float* ggamma_dev, float* gbeta_dev, void* ws_dev, int64_t ws_bytes,
                      void* stream) {
  if (!gy_dev || !x_dev || !offsets_dev || !z_dev || !w_dev || !gw_dev)
    return fail(nullptr, XV_ERR_INVALID, "xv_gconv_backward: null pointer");
  int rc = gconv_check("xv_gconv_backward", channels, bins, kh, kw, st, sf, out_dim, batch, total_in, total_out, ldx, ldw, gamma_dev,
                       beta_dev, mean_dev, var_dev, act);
  if (rc != XV_OK) return rc;
  if (gamma_dev && (!ggamma_dev || !gbeta_dev))
    return fail(nullptr, XV_ERR_INVALID, "xv_gconv_backward: batch norm needs ggamma_dev and gbeta_dev");
  if (ldgy < out_dim || ldz < out_dim || (gx_dev && ldgx < channels))
    return fail(nullptr, XV_ERR_INVALID, "xv_gconv_backward: bad dimensions");
  if (batch == 0 || total_out == 0) return XV_OK;
  if (total_in < 1) return fail(nullptr, XV_ERR_INVALID, "xv_gconv_backward: output frames without input frames");
  if ((rc = layer_ws_check("xv_gconv_backward", ws_dev, ws_bytes,
                           gconv_workspace_bytes(batch, total_in, total_out, bins, kh, kw, st, sf, channels, out_dim))) != XV_OK)
    return rc;
  return with_device(device, "xv_gconv_backward", [&] {
    return launch_gconv_backward(gy_dev, ldgy, x_dev, ldx, channels, bins, kh, kw, st, sf, offsets_dev, batch, total_in, total_out,
                                 z_dev, ldz, w_dev, ldw, out_dim, gamma_dev, beta_dev, mean_dev, var_dev, act, gx_dev, ldgx, gw_dev,
                                 gbias_dev, ggamma_dev, gbeta_dev, ws_dev, to_stream(stream));
  });
}

namespace {

int add_act_check(const char* op, int64_t rows, int out_dim, int64_t ldp, int64_t ldq, int64_t ldo, int act) {
  if (rows > ((int64_t)1 << 28) || out_dim > 65536)
    return fail(nullptr, XV_ERR_UNSUPPORTED, "%s: rows <= 2^28, out_dim <= 65536, got %lld, %d", op, (long long)rows, out_dim);
  if (rows < 0 || out_dim < 1 || ldp < out_dim || ldq < out_dim || ldo < out_dim) return fail(nullptr, XV_ERR_INVALID, "%s: bad dimensions", op);
  if (act < XV_SEG_ACT_NONE || act > XV_SEG_ACT_LRELU) return fail(nullptr, XV_ERR_INVALID, "%s: unknown activation %d", op, act);
  return XV_OK;
}

}  // namespace

int xv_add_act_forward(int device, const float* p_dev, int64_t ldp, const float* q_dev, int64_t ldq, int64_t rows, int out_dim, int act,
                       float* y_dev, int64_t ldy, void* stream) {
  const int rc = add_act_check("xv_add_act_forward", rows, out_dim, ldp, ldq, ldy, act);
  if (rc != XV_OK) return rc;
  if (rows == 0) return XV_OK;
  if (!p_dev || !q_dev || !y_dev) return fail(nullptr, XV_ERR_INVALID, "xv_add_act_forward: null pointer");
  return with_device(device, "xv_add_act_forward", [&] {
    return launch_add_act(nullptr, 0, p_dev, ldp, q_dev, ldq, rows, out_dim, act, y_dev, ldy, to_stream(stream));
  });
}

int xv_add_act_backward(int device, const float* gy_dev, int64_t ldgy, const float* p_dev, int64_t ldp, const float* q_dev, int64_t ldq,
                        int64_t rows, int out_dim, int act, float* g_dev, int64_t ldg, void* stream) {
  const int rc = add_act_check("xv_add_act_backward", rows, out_dim, ldp, ldq, ldg, act);
  if (rc != XV_OK) return rc;
  if (ldgy < out_dim) return fail(nullptr, XV_ERR_INVALID, "xv_add_act_backward: bad dimensions");
  if (rows == 0) return XV_OK;
  if (!gy_dev || !p_dev || !q_dev || !g_dev) return fail(nullptr, XV_ERR_INVALID, "xv_add_act_backward: null pointer");
  return with_device(device, "xv_add_act_backward", [&] {
    return launch_add_act(gy_dev, ldgy, p_dev, ldp, q_dev, ldq, rows, out_dim, act, g_dev, ldg, to_stream(stream));
  });
}

// batch norm in training mode on a stored product z (include/xvec_hip.h, csrc/bn_batch.hip)
int64_t xv_bn_batch_workspace(int64_t n, int out_dim) { return bn_batch_workspace_bytes(n, out_dim); }

int64_t xv_bn_batch_workspace_min(int64_t n, int out_dim) { return bn_batch_workspace_bytes(n, out_dim); }

namespace {

// the checks the two batch-statistics calls share; `op` names the caller in the message
int bn_batch_check(const char* op, int64_t n, int out_dim, int64_t ldz, int64_t ldo, int act) {
  if (out_dim > 4096 || n > (1 << 24))
    return fail(nullptr, XV_ERR_UNSUPPORTED, "%s: out_dim <= 4096, n <= 2^24, got %d, %lld", op, out_dim, (long long)n);
  if (n < 1 || out_dim < 1 || ldz < out_dim || ldo < out_dim) return fail(nullptr, XV_ERR_INVALID, "%s: bad dimensions", op);
  if (act < XV_SEG_ACT_NONE || act > XV_SEG_ACT_LRELU) return fail(nullptr, XV_ERR_INVALID, "%s: unknown activation %d", op, act);
  return XV_OK;
}

}  // namespace

int xv_bn_batch_forward(int device, const float* z_dev, int64_t ldz, int64_t n, int out_dim, const float* gamma_dev,
                        const float* beta_dev, int act, double momentum, int bessel, float* moving_mean_dev, float* moving_var_dev,
                        float* y_dev, int64_t ldy, float* batch_mean_dev, float* batch_var_dev, void* ws_dev, int64_t ws_bytes,
                        void* stream) {
  if (!z_dev || !gamma_dev || !beta_dev || !y_dev || !batch_mean_dev || !batch_var_dev)
    return fail(nullptr, XV_ERR_INVALID, "xv_bn_batch_forward: null pointer");
  if ((moving_mean_dev != nullptr) != (moving_var_dev != nullptr))
    return fail(nullptr, XV_ERR_INVALID, "xv_bn_batch_forward: moving_mean and moving_variance, or neither");
  int rc = bn_batch_check("xv_bn_batch_forward", n, out_dim, ldz, ldy, act);
  if (rc != XV_OK) return rc;
  if (!(momentum >= 0.0 && momentum <= 1.0)) return fail(nullptr, XV_ERR_INVALID, "xv_bn_batch_forward: 0 <= momentum <= 1");
  if ((rc = layer_ws_check("xv_bn_batch_forward", ws_dev, ws_bytes, bn_batch_workspace_bytes(n, out_dim))) != XV_OK) return rc;
  return with_device(device, "xv_bn_batch_forward", [&] {
    return launch_bn_batch_forward(z_dev, ldz, n, out_dim, gamma_dev, beta_dev, act, momentum, bessel ? 1 : 0, moving_mean_dev,
                                   moving_var_dev, y_dev, ldy, batch_mean_dev, batch_var_dev, ws_dev, to_stream(stream));
  });
}

int xv_bn_batch_backward(int device, const float* gy_dev, int64_t ldgy, const float* z_dev, int64_t ldz, int64_t n, int out_dim,
                         const float* batch_mean_dev, const float* batch_var_dev, const float* gamma_dev, const float* beta_dev,
                         int act, float* gz_dev, int64_t ldgz, float* ggamma_dev, float* gbeta_dev, void* ws_dev, int64_t ws_bytes,
                         void* stream) {
  if (!gy_dev || !z_dev || !batch_mean_dev || !batch_var_dev || !gamma_dev || !beta_dev || !gz_dev || !ggamma_dev || !gbeta_dev)
    return fail(nullptr, XV_ERR_INVALID, "xv_bn_batch_backward: null pointer");
  int rc = bn_batch_check("xv_bn_batch_backward", n, out_dim, ldz, ldgz, act);
  if (rc != XV_OK) return rc;
  if (ldgy < out_dim) return fail(nullptr, XV_ERR_INVALID, "xv_bn_batch_backward: bad dimensions");
  if ((rc = layer_ws_check("xv_bn_batch_backward", ws_dev, ws_bytes, bn_batch_workspace_bytes(n, out_dim))) != XV_OK) return rc;
  return with_device(device, "xv_bn_batch_backward", [&] {
    return launch_bn_batch_backward(gy_dev, ldgy, z_dev, ldz, n, out_dim, batch_mean_dev, batch_var_dev, gamma_dev, beta_dev, act,
                                    gz_dev, ldgz, ggamma_dev, gbeta_dev, ws_dev, to_stream(stream));
  });
}

int xv_plda_prepare(int device, const float* x_dev, int64_t ldx, int64_t n, int d_in, const float* transform_dev, int64_t ldt,
                    int d, int norm, int side, int pack_second, const double* tables_dev, const double* logdet_dev,
                    int num_tables, const int32_t* table_index_dev, float* rows_dev, int64_t ldr, float* packed_dev, int64_t ldp,
                    float* bias_dev, void* stream) {
  if (!x_dev || !tables_dev) return fail(nullptr, XV_ERR_INVALID, "xv_plda_prepare: null pointer");
  if (d < 1 || d > 2048 || d_in < 1 || d_in > 2048)
    return fail(nullptr, XV_ERR_UNSUPPORTED, "xv_plda_prepare: 1 <= d, d_in <= 2048, got %d, %d", d, d_in);
  if (n < 0 || n > INT32_MAX || ldx < d_in || num_tables < 1 || norm < 0 || norm > 2 || side < 0 || side > 1)
    return fail(nullptr, XV_ERR_INVALID, "xv_plda_prepare: bad dimensions");
  if (rows_dev && ldr < d) return fail(nullptr, XV_ERR_INVALID, "xv_plda_prepare: bad dimensions");
  if (packed_dev && (ldp < (pack_second ? 2 * (int64_t)d : d) || packed_dev == x_dev || packed_dev == rows_dev))
    return fail(nullptr, XV_ERR_INVALID, "xv_plda_prepare: packed rows of dimension %d need a buffer of their own with ldp >= %d", d,
                pack_second ? 2 * d : d);
  if (transform_dev) {
    if (ldt < d_in + 1) return fail(nullptr, XV_ERR_INVALID, "xv_plda_prepare: the transform is [d, d_in + 1] (last column: offset)");
    if (!rows_dev || rows_dev == x_dev) return fail(nullptr, XV_ERR_INVALID, "xv_plda_prepare: a transform needs rows_dev, not in place");
  } else if (d_in != d) {
    return fail(nullptr, XV_ERR_INVALID, "xv_plda_prepare: d_in != d without a transform");
  }
  return with_device(device, "plda_prepare", [&] {
    hipStream_t s = to_stream(stream);
    hipError_t e = hipSuccess;
    const float* u = x_dev;
    int64_t ldu = ldx;
    if (transform_dev) {
      e = launch_score_matrix(x_dev, ldx, (int)n, transform_dev, ldt, d, d_in, nullptr, 1, rows_dev, ldr, s);
      u = rows_dev;
      ldu = ldr;
    }
    if (e == hipSuccess)
      e = launch_plda_rows(u, ldu, n, d, norm, side, pack_second ? 1 : 0, tables_dev, logdet_dev, table_index_dev, num_tables, rows_dev,
                           ldr, packed_dev, ldp, bias_dev, s);
    return e;
  });
}

// shared argument check of the three PLDA scoring entry points: packed rows a [n, k], b [m, k], rho [n], tau [m] or null
static int plda_operands(const char* who, const float* a, int64_t lda, int64_t n, const float* rho, const float* b, int64_t ldb,
                         int64_t m, int k) {
  if (const int rc = score_operands(who, a, lda, n, b, ldb, m, k)) return rc;
  if (!rho) return fail(nullptr, XV_ERR_INVALID, "%s: null pointer", who);
  return XV_OK;
}

int xv_plda_matrix(int device, const float* a_dev, int64_t lda, int64_t n, const float* rho_dev, const float* b_dev, int64_t ldb,
                   int64_t m, const float* tau_dev, int k, float* out_dev, int64_t ldo, void* stream) {
  if (const int rc = plda_operands("xv_plda_matrix", a_dev, lda, n, rho_dev, b_dev, ldb, m, k)) return rc;
  if (!out_dev || ldo < m) return fail(nullptr, XV_ERR_INVALID, "xv_plda_matrix: bad output");
  return with_device(device, "plda_matrix", [&] {
    return launch_plda_matrix(a_dev, lda, (int)n, rho_dev, b_dev, ldb, (int)m, tau_dev, k, out_dev, ldo,
                              to_stream(stream));
  });
}

int xv_plda_pairs(int device, const float* a_dev, int64_t lda, int64_t n, const float* rho_dev, const float* b_dev, int64_t ldb,
                  int64_t m, const float* tau_dev, int k, const int32_t* ia_dev, const int32_t* ib_dev, int64_t npairs,
                  float* out_dev, void* stream) {
  if (const int rc = plda_operands("xv_plda_pairs", a_dev, lda, n, rho_dev, b_dev, ldb, m, k)) return rc;
  if (npairs < 0 || npairs > ((int64_t)1 << 34)) return fail(nullptr, XV_ERR_INVALID, "xv_plda_pairs: bad pair count");
  if (npairs > 0 && (!ia_dev || !ib_dev || !out_dev)) return fail(nullptr, XV_ERR_INVALID, "xv_plda_pairs: null pointer");
  return with_device(device, "plda_pairs", [&] {
    return launch_plda_pairs(a_dev, lda, (int)n, rho_dev, b_dev, ldb, (int)m, tau_dev, k, ia_dev, ib_dev, npairs, out_dev,
                             to_stream(stream));
  });
}

int xv_plda_histogram(int device, const float* a_dev, int64_t lda, int64_t n, const float* rho_dev, const int32_t* labels_a_dev,
                      const float* b_dev, int64_t ldb, int64_t m, const float* tau_dev, const int32_t* labels_b_dev, int k, double lo,
                      double hi, int nbins, uint64_t* hist_same_dev, uint64_t* hist_diff_dev, void* stream) {
  if (const int rc = plda_operands("xv_plda_histogram", a_dev, lda, n, rho_dev, b_dev, ldb, m, k)) return rc;
  if (const int rc = check_nbins("xv_plda_histogram", nbins)) return rc;
  if (!(lo < hi) || !(hi - lo <= 1.7976931348623157e308))
    return fail(nullptr, XV_ERR_INVALID, "xv_plda_histogram: the range [lo, hi) is empty or not finite");
  if (!labels_a_dev || !labels_b_dev || !hist_same_dev || !hist_diff_dev || hist_same_dev == hist_diff_dev)
    return fail(nullptr, XV_ERR_INVALID, "xv_plda_histogram: null pointer");
  return with_device(device, "plda_histogram", [&] {
    return launch_plda_histogram(a_dev, lda, (int)n, rho_dev, labels_a_dev, b_dev, ldb, (int)m, tau_dev, labels_b_dev, k, lo,
                                 hi, nbins, reinterpret_cast<unsigned long long*>(hist_same_dev),
                                 reinterpret_cast<unsigned long long*>(hist_diff_dev), to_stream(stream));
  });
}

// shared argument checks of the two panel entry points (xv_cohort_stats, xv_score_topk)
static int exclusion_labels(const char* who, const int32_t* la, const int32_t* lb) {
  if ((la == nullptr) != (lb == nullptr))
    return fail(nullptr, XV_ERR_INVALID, "%s: exclusion labels are given for both sides or for neither", who);
  return XV_OK;
}

static int panel_workspace(const char* who, const void* ws, int64_t ws_bytes, int64_t need) {
  if (ws_bytes < need || !ws)
    return fail(nullptr, XV_ERR_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", who, (long long)(ws ? ws_bytes : 0), (long long)need);
  return XV_OK;
}

int64_t xv_cohort_stats_workspace(int64_t n, int64_t m, int top_k) {
  if (n < 0 || m < 0 || m > INT32_MAX || top_k < 0) return XV_ERR_INVALID;
  return cohort_stats_workspace_bytes(n, m);
}

int xv_cohort_stats(int device, const float* a_dev, int64_t lda, int64_t n, const float* row_bias_dev, const int32_t* labels_a_dev,
                    const float* b_dev, int64_t ldb, int64_t m, const float* col_bias_dev, const int32_t* labels_b_dev, int k,
                    int top_k, float* mean_dev, float* std_dev, int32_t* count_dev, void* ws_dev, int64_t ws_bytes, void* stream) {
  if (const int rc = score_operands("xv_cohort_stats", a_dev, lda, n, b_dev, ldb, m, k)) return rc;
  if (top_k < 0 || top_k > m) return fail(nullptr, XV_ERR_INVALID, "xv_cohort_stats: 0 <= top_k <= m, got %d for m = %lld", top_k, (long long)m);
  if (const int rc = exclusion_labels("xv_cohort_stats", labels_a_dev, labels_b_dev)) return rc;
  if (n == 0) return XV_OK;
  if (!mean_dev || !std_dev) return fail(nullptr, XV_ERR_INVALID, "xv_cohort_stats: null pointer");
  if (const int rc = panel_workspace("xv_cohort_stats", ws_dev, ws_bytes, cohort_stats_workspace_bytes(n, m))) return rc;
  return with_device(device, "cohort_stats", [&] {
    return launch_cohort_stats(a_dev, lda, (int)n, row_bias_dev, labels_a_dev, b_dev, ldb, (int)m, col_bias_dev, labels_b_dev,
                               k, top_k, mean_dev, std_dev, count_dev, ws_dev, ws_bytes, to_stream(stream));
  });
}

int64_t xv_score_topk_workspace(int64_t n, int64_t m, int top_k) {
  if (n < 0 || m < 0 || m > INT32_MAX || top_k < 1 || top_k > 1024) return XV_ERR_INVALID;
  return score_topk_workspace_bytes(n, m);
}

int xv_score_topk(int device, const float* a_dev, int64_t lda, int64_t n, const float* row_bias_dev, const int32_t* labels_a_dev,
                  const float* b_dev, int64_t ldb, int64_t m, const float* col_bias_dev, const int32_t* labels_b_dev, int k, int top_k,
                  float* scores_dev, int32_t* index_dev, int64_t ldo, int32_t* count_dev, void* ws_dev, int64_t ws_bytes,
                  void* stream) {
  if (const int rc = score_operands("xv_score_topk", a_dev, lda, n, b_dev, ldb, m, k)) return rc;
  if (top_k < 1 || top_k > 1024) return fail(nullptr, XV_ERR_UNSUPPORTED, "xv_score_topk: 1 <= top_k <= 1024, got %d", top_k);
  if (ldo < top_k) return fail(nullptr, XV_ERR_INVALID, "xv_score_topk: ldo = %lld for top_k = %d", (long long)ldo, top_k);
  if (const int rc = exclusion_labels("xv_score_topk", labels_a_dev, labels_b_dev)) return rc;
  if (n == 0) return XV_OK;
  if (!scores_dev || !index_dev) return fail(nullptr, XV_ERR_INVALID, "xv_score_topk: null pointer");
  if (const int rc = panel_workspace("xv_score_topk", ws_dev, ws_bytes, score_topk_workspace_bytes(n, m))) return rc;
  return with_device(device, "score_topk", [&] {
    return launch_score_topk(a_dev, lda, (int)n, row_bias_dev, labels_a_dev, b_dev, ldb, (int)m, col_bias_dev, labels_b_dev, k,
                             top_k, scores_dev, index_dev, ldo, count_dev, ws_dev, ws_bytes, to_stream(stream));
  });
}

int64_t xv_ahc_matrix_floats(int64_t n) { return ahc_matrix_floats(n); }

int64_t xv_ahc_workspace(int64_t num_groups, const int32_t* rows_host) {
  if (num_groups < 0 || num_groups > INT32_MAX || (num_groups > 0 && !rows_host)) return XV_ERR_INVALID;
  for (int64_t g = 0; g < num_groups; ++g) {      // group by group, as xv_ahc does
    if (rows_host[g] < 0) return XV_ERR_INVALID;
    if (rows_host[g] > 8192) return XV_ERR_UNSUPPORTED;
  }
  return ahc_workspace_bytes(num_groups);
}

int xv_ahc(int device, float* s_dev, const int32_t* rows_host, const int32_t* target_host, int64_t num_groups, double threshold,
           int32_t* labels_dev, int32_t* num_clusters_dev, int32_t* merge_a_dev, int32_t* merge_b_dev, double* merge_height_dev,
           void* ws_dev, int64_t ws_bytes, void* stream) {
  if (num_groups < 0 || num_groups > INT32_MAX) return fail(nullptr, XV_ERR_INVALID, "xv_ahc: bad group count %lld", (long long)num_groups);
  if (num_groups == 0) return XV_OK;
  if (!rows_host) return fail(nullptr, XV_ERR_INVALID, "xv_ahc: null pointer");
  if (threshold != threshold) return fail(nullptr, XV_ERR_INVALID, "xv_ahc: the threshold is NaN (-inf means none)");
  int64_t total = 0;
  for (int64_t g = 0; g < num_groups; ++g) {
    if (rows_host[g] < 0) return fail(nullptr, XV_ERR_INVALID, "xv_ahc: group %lld has %d rows", (long long)g, rows_host[g]);
    if (rows_host[g] > 8192)
      return fail(nullptr, XV_ERR_UNSUPPORTED, "xv_ahc: group %lld has %d rows, at most 8192", (long long)g, rows_host[g]);
    if (target_host && target_host[g] < 1)
      return fail(nullptr, XV_ERR_INVALID, "xv_ahc: group %lld has target %d, at least 1", (long long)g, target_host[g]);
    total += rows_host[g];
  }
  if (!num_clusters_dev || (total > 0 && (!s_dev || !labels_dev || !merge_a_dev || !merge_b_dev || !merge_height_dev)))
    return fail(nullptr, XV_ERR_INVALID, "xv_ahc: null pointer");
  const int64_t need = ahc_workspace_bytes(num_groups);
  if (ws_bytes < need || !ws_dev)
    return fail(nullptr, XV_ERR_WORKSPACE, "xv_ahc: workspace of %lld bytes, %lld needed", (long long)(ws_dev ? ws_bytes : 0), (long long)need);
  if (reinterpret_cast<uintptr_t>(ws_dev) & 7)
    return fail(nullptr, XV_ERR_INVALID, "xv_ahc: the workspace must be 8-byte aligned (it holds the group table)");
  return with_device(device, "xv_ahc", [&] {
    return launch_ahc(s_dev, rows_host, target_host, num_groups, threshold, labels_dev, num_clusters_dev, merge_a_dev,
                      merge_b_dev, merge_height_dev, ws_dev, to_stream(stream));
  });
}

int64_t xv_plda_adapt_workspace(int64_t num_groups, int d) {
  if (d < 1 || d > 256) return XV_ERR_UNSUPPORTED;
  if (num_groups < 0 || num_groups > INT32_MAX) return XV_ERR_INVALID;
  return plda_adapt_workspace_bytes(num_groups, d);
}

int64_t xv_plda_adapt_slot_bytes(int d) {
  if (d < 1 || d > 256) return XV_ERR_UNSUPPORTED;
  return plda_adapt_slot_bytes(d);
}

int xv_plda_adapt(int device, const float* x_dev, int64_t ldx, const int64_t* offsets_host, int64_t num_groups, int d,
                  const double* mean_dev, const double* within_factor_dev, const double* psi_dev, double target_energy,
                  int32_t* dim_dev, double* eigval_dev, double* pca_dev, double* affine_dev, double* psi_out_dev, void* ws_dev,
                  int64_t ws_bytes, void* stream) {
  if (d < 1 || d > 256) return fail(nullptr, XV_ERR_UNSUPPORTED, "xv_plda_adapt: 1 <= d <= 256, got %d", d);
  if (!(target_energy > 0.0 && target_energy <= 1.0))
    return fail(nullptr, XV_ERR_INVALID, "xv_plda_adapt: target_energy must be in (0, 1], got %g", target_energy);
  if (num_groups < 0 || num_groups > INT32_MAX)
    return fail(nullptr, XV_ERR_INVALID, "xv_plda_adapt: bad group count %lld", (long long)num_groups);
  if (num_groups == 0) return XV_OK;
  if (!offsets_host || ldx < d) return fail(nullptr, XV_ERR_INVALID, "xv_plda_adapt: bad arguments (offsets, ldx >= d)");
  if (offsets_host[0] < 0) return fail(nullptr, XV_ERR_INVALID, "xv_plda_adapt: the first offset is negative");
  for (int64_t g = 0; g < num_groups; ++g)
    if (offsets_host[g + 1] < offsets_host[g])
      return fail(nullptr, XV_ERR_INVALID, "xv_plda_adapt: the offsets decrease at group %lld", (long long)g);
  if (!mean_dev || !within_factor_dev || !psi_dev || !dim_dev || !eigval_dev || !pca_dev || !affine_dev || !psi_out_dev ||
      (offsets_host[num_groups] > 0 && !x_dev))
    return fail(nullptr, XV_ERR_INVALID, "xv_plda_adapt: null pointer");
  const int64_t need = plda_adapt_workspace_bytes(num_groups, d);
  if (ws_bytes < need || !ws_dev)
    return fail(nullptr, XV_ERR_WORKSPACE, "xv_plda_adapt: workspace of %lld bytes, %lld needed", (long long)(ws_dev ? ws_bytes : 0),
                (long long)need);
  if (reinterpret_cast<uintptr_t>(ws_dev) & 7)
    return fail(nullptr, XV_ERR_INVALID, "xv_plda_adapt: the workspace must be 8-byte aligned (it holds offsets and doubles)");
  return with_device(device, "xv_plda_adapt", [&] {
    return launch_plda_adapt(x_dev, ldx, offsets_host, num_groups, d, mean_dev, within_factor_dev, psi_dev, target_energy, dim_dev,
                             eigval_dev, pca_dev, affine_dev, psi_out_dev, ws_dev, ws_bytes, to_stream(stream));
  });
}

// shared argument check of the two VB-HMM entry points: the group table
static int vbx_groups(const char* who, int64_t num_groups, const int64_t* offsets_host, const int32_t* num_spk_host, int r) {
  if (r < 1 || r > 256) return fail(nullptr, XV_ERR_UNSUPPORTED, "%s: 1 <= r <= 256, got %d", who, r);
  if (num_groups < 0 || num_groups > INT32_MAX) return fail(nullptr, XV_ERR_INVALID, "%s: bad group count %lld", who, (long long)num_groups);
  if (num_groups == 0) return XV_OK;
  if (!offsets_host || !num_spk_host) return fail(nullptr, XV_ERR_INVALID, "%s: null pointer", who);
  if (offsets_host[0] < 0) return fail(nullptr, XV_ERR_INVALID, "%s: the first offset is negative", who);
  for (int64_t g = 0; g < num_groups; ++g) {
    if (offsets_host[g + 1] < offsets_host[g]) return fail(nullptr, XV_ERR_INVALID, "%s: the offsets decrease at group %lld", who, (long long)g);
    if (offsets_host[g + 1] - offsets_host[g] > 8192)
      return fail(nullptr, XV_ERR_UNSUPPORTED, "%s: group %lld has %lld rows, at most 8192", who, (long long)g,
                  (long long)(offsets_host[g + 1] - offsets_host[g]));
    if (num_spk_host[g] < 1 || num_spk_host[g] > 64)
      return fail(nullptr, XV_ERR_UNSUPPORTED, "%s: group %lld has %d speakers, 1 .. 64", who, (long long)g, num_spk_host[g]);
  }
  return XV_OK;
}

int64_t xv_vbx_workspace(int64_t num_groups, const int64_t* offsets_host, const int32_t* num_spk_host, int r) {
  if (const int rc = vbx_groups("xv_vbx_workspace", num_groups, offsets_host, num_spk_host, r)) return rc;
  if (num_groups == 0) return 0;
  return vbx_workspace_bytes(num_groups, offsets_host, num_spk_host, r);
}

int xv_vbx(int device, const float* x_dev, int64_t ldx, const int64_t* offsets_host, const int32_t* num_spk_host, int64_t num_groups,
           int d, const double* affine_dev, const double* psi_dev, int r, double* gamma_dev, double* pi_dev, double fa, double fb,
           double loop_prob, int max_iters, double epsilon, int32_t* labels_dev, double* elbo_dev, int32_t* iters_dev, void* ws_dev,
           int64_t ws_bytes, void* stream) {
  if (d < 1 || d > 2048) return fail(nullptr, XV_ERR_UNSUPPORTED, "xv_vbx: 1 <= d <= 2048, got %d", d);
  if (const int rc = vbx_groups("xv_vbx", num_groups, offsets_host, num_spk_host, r)) return rc;
  if (!(fa > 0.0) || !(fb > 0.0) || fa > DBL_MAX || fb > DBL_MAX)
    return fail(nullptr, XV_ERR_INVALID, "xv_vbx: Fa and Fb must be positive and finite, got %g, %g", fa, fb);
  if (!(loop_prob >= 0.0 && loop_prob <= 1.0)) return fail(nullptr, XV_ERR_INVALID, "xv_vbx: loop_prob must be in [0, 1], got %g", loop_prob);
  if (max_iters < 1) return fail(nullptr, XV_ERR_INVALID, "xv_vbx: max_iters must be >= 1, got %d", max_iters);
  if (epsilon != epsilon) return fail(nullptr, XV_ERR_INVALID, "xv_vbx: epsilon is NaN (-inf means: run max_iters iterations)");
  if (num_groups == 0) return XV_OK;
  if (ldx < d) return fail(nullptr, XV_ERR_INVALID, "xv_vbx: ldx = %lld for d = %d", (long long)ldx, d);
  if (!affine_dev || !psi_dev || !iters_dev ||
      (offsets_host[num_groups] > offsets_host[0] && (!x_dev || !gamma_dev || !pi_dev || !labels_dev || !elbo_dev)))
    return fail(nullptr, XV_ERR_INVALID, "xv_vbx: null pointer");
  const int64_t need = vbx_workspace_bytes(num_groups, offsets_host, num_spk_host, r);
  if (ws_bytes < need || !ws_dev)
    return fail(nullptr, XV_ERR_WORKSPACE, "xv_vbx: workspace of %lld bytes, %lld needed", (long long)(ws_dev ? ws_bytes : 0), (long long)need);
  if (reinterpret_cast<uintptr_t>(ws_dev) & 7)
    return fail(nullptr, XV_ERR_INVALID, "xv_vbx: the workspace must be 8-byte aligned (it holds the group table and doubles)");
  return with_device(device, "xv_vbx", [&] {
    return launch_vbx(x_dev, ldx, offsets_host, num_spk_host, num_groups, d, affine_dev, psi_dev, r, gamma_dev, pi_dev, fa, fb, loop_prob,
                      max_iters, epsilon, labels_dev, elbo_dev, iters_dev, ws_dev, to_stream(stream));
  });
}

// shared argument check of the two metric-loss entry points
static int metric_groups(const char* who, int64_t num_groups, const int64_t* offsets_host, int d, int kind) {
  if (kind < XV_METRIC_SEMIHARD || kind > XV_METRIC_GE2E_CONTRASTIVE) return fail(nullptr, XV_ERR_INVALID, "%s: unknown kind %d", who, kind);
  if (d < 1 || d > 4096) return fail(nullptr, XV_ERR_INVALID, "%s: 1 <= d <= 4096, got %d", who, d);
  if (num_groups < 0 || num_groups > INT32_MAX) return fail(nullptr, XV_ERR_INVALID, "%s: bad group count %lld", who, (long long)num_groups);
  if (num_groups == 0) return XV_OK;
  if (!offsets_host) return fail(nullptr, XV_ERR_INVALID, "%s: null pointer", who);
  if (offsets_host[0] < 0) return fail(nullptr, XV_ERR_INVALID, "%s: the first offset is negative", who);
  for (int64_t g = 0; g < num_groups; ++g) {
    const int64_t rows = offsets_host[g + 1] - offsets_host[g];
    if (rows < 1 || rows > 4096)
      return fail(nullptr, XV_ERR_INVALID, "%s: group %lld has %lld rows (1 .. 4096; the offsets ascend)", who, (long long)g, (long long)rows);
  }
  return XV_OK;
}

int64_t xv_metric_loss_workspace(int64_t num_groups, const int64_t* offsets_host, int d, int kind) {
  if (const int rc = metric_groups("xv_metric_loss_workspace", num_groups, offsets_host, d, kind)) return rc;
  if (num_groups == 0) return 0;
  return metric_loss_workspace_bytes(num_groups, offsets_host, d, kind);
}

int64_t xv_metric_loss_slot_bytes(int max_rows, int d, int kind) {
  const int64_t offsets[2] = {0, max_rows};
  if (const int rc = metric_groups("xv_metric_loss_slot_bytes", 1, offsets, d, kind)) return rc;
  return metric_loss_slot_bytes(max_rows, d, kind);
}

int xv_metric_loss(int device, const float* x_dev, int64_t ldx, const int64_t* offsets_host, int64_t num_groups, int d,
                   const int32_t* labels_dev, int kind, int pos_head, double margin, int squared, int normalize, double w, double b,
                   double* row_loss_dev, int64_t* row_count_dev, int32_t* row_top1_dev, double* group_loss_dev,
                   int64_t* group_count_dev, void* ws_dev, int64_t ws_bytes, void* stream) {
  if (const int rc = metric_groups("xv_metric_loss", num_groups, offsets_host, d, kind)) return rc;
  if (num_groups == 0) return XV_OK;
  if (!x_dev || !labels_dev || !row_loss_dev || !row_count_dev || !group_loss_dev || !group_count_dev)
    return fail(nullptr, XV_ERR_INVALID, "xv_metric_loss: null pointer");
  if (ldx < d) return fail(nullptr, XV_ERR_INVALID, "xv_metric_loss: ldx = %lld < d = %d", (long long)ldx, d);
  if (!std::isfinite(margin) || !std::isfinite(w) || !std::isfinite(b)) return fail(nullptr, XV_ERR_INVALID, "xv_metric_loss: margin, w and b must be finite");
  if (kind == XV_METRIC_ANGULAR_ALL || kind == XV_METRIC_ANGULAR_HARD) {
    if (pos_head < XV_LOSS_ASOFTMAX || pos_head > XV_LOSS_ARCSOFTMAX) return fail(nullptr, XV_ERR_INVALID, "xv_metric_loss: unknown pos_head %d", pos_head);
    if (pos_head == XV_LOSS_ASOFTMAX && margin != 1.0 && margin != 2.0 && margin != 4.0)
      return fail(nullptr, XV_ERR_UNSUPPORTED, "xv_metric_loss: m=%g is not supported (asoftmax: 1, 2 or 4)", margin);   // loss.py:168
  }
  const int64_t need = metric_loss_workspace_bytes(num_groups, offsets_host, d, kind);
  if (ws_bytes < need || !ws_dev)
    return fail(nullptr, XV_ERR_WORKSPACE, "xv_metric_loss: workspace of %lld bytes, %lld needed", (long long)(ws_dev ? ws_bytes : 0),
                (long long)need);
  if (reinterpret_cast<uintptr_t>(ws_dev) & 7)
    return fail(nullptr, XV_ERR_INVALID, "xv_metric_loss: the workspace must be 8-byte aligned (it holds offsets and doubles)");
  return with_device(device, "xv_metric_loss", [&] {
    return launch_metric_loss(x_dev, ldx, offsets_host, num_groups, d, labels_dev, kind, pos_head, margin, squared ? 1 : 0,
                              normalize ? 1 : 0, w, b, row_loss_dev, row_count_dev, row_top1_dev, group_loss_dev, group_count_dev,
                              ws_dev, ws_bytes, to_stream(stream));
  });
}

// kinds and group sizes of the gradient: the forward's checks, then what only the gradient refuses
static int metric_grad_groups(const char* who, int64_t num_groups, const int64_t* offsets_host, int d, int kind) {
  if (const int rc = metric_groups(who, num_groups, offsets_host, d, kind)) return rc;
  if (kind > XV_METRIC_ANGULAR_HARD)
    return fail(nullptr, XV_ERR_UNSUPPORTED, "%s: kind %d has no gradient (the triplet kinds 0 .. 2 have)", who, kind);
  for (int64_t g = 0; g < num_groups; ++g)
    if (offsets_host[g + 1] - offsets_host[g] > 1024)
      return fail(nullptr, XV_ERR_UNSUPPORTED, "%s: group %lld has %lld rows (the gradient takes 1 .. 1024)", who, (long long)g,
                  (long long)(offsets_host[g + 1] - offsets_host[g]));
  return XV_OK;
}

int64_t xv_metric_loss_grad_workspace(int64_t num_groups, const int64_t* offsets_host, int d, int kind) {
  if (const int rc = metric_grad_groups("xv_metric_loss_grad_workspace", num_groups, offsets_host, d, kind)) return rc;
  if (num_groups == 0) return 0;
  return metric_loss_grad_workspace_bytes(num_groups, offsets_host, d);
}

int xv_metric_loss_grad(int device, const float* x_dev, int64_t ldx, const int64_t* offsets_host, int64_t num_groups, int d,
                        const int32_t* labels_dev, int kind, int pos_head, double margin, int squared, int normalize,
                        double grad_scale, double* row_loss_dev, int64_t* row_count_dev, double* group_loss_dev,
                        int64_t* group_count_dev, float* grad_x_dev, int64_t ldg, void* ws_dev, int64_t ws_bytes, void* stream) {
  if (const int rc = metric_grad_groups("xv_metric_loss_grad", num_groups, offsets_host, d, kind)) return rc;
  if (num_groups == 0) return XV_OK;
  if (!x_dev || !labels_dev || !row_loss_dev || !row_count_dev || !group_loss_dev || !group_count_dev || !grad_x_dev)
    return fail(nullptr, XV_ERR_INVALID, "xv_metric_loss_grad: null pointer");
  if (ldx < d) return fail(nullptr, XV_ERR_INVALID, "xv_metric_loss_grad: ldx = %lld < d = %d", (long long)ldx, d);
  if (ldg < d) return fail(nullptr, XV_ERR_INVALID, "xv_metric_loss_grad: ldg = %lld < d = %d", (long long)ldg, d);
  if (!std::isfinite(margin) || !std::isfinite(grad_scale))
    return fail(nullptr, XV_ERR_INVALID, "xv_metric_loss_grad: margin and grad_scale must be finite");
  if (kind == XV_METRIC_ANGULAR_ALL || kind == XV_METRIC_ANGULAR_HARD) {
    if (pos_head < XV_LOSS_ASOFTMAX || pos_head > XV_LOSS_ARCSOFTMAX)
      return fail(nullptr, XV_ERR_INVALID, "xv_metric_loss_grad: unknown pos_head %d", pos_head);
    if (pos_head == XV_LOSS_ASOFTMAX && margin != 1.0 && margin != 2.0 && margin != 4.0)
      return fail(nullptr, XV_ERR_UNSUPPORTED, "xv_metric_loss_grad: m=%g is not supported (asoftmax: 1, 2 or 4)", margin);
  }
  const int64_t need = metric_loss_grad_workspace_bytes(num_groups, offsets_host, d);
  if (ws_bytes < need || !ws_dev)
    return fail(nullptr, XV_ERR_WORKSPACE, "xv_metric_loss_grad: workspace of %lld bytes, %lld needed", (long long)(ws_dev ? ws_bytes : 0),
                (long long)need);
  if (reinterpret_cast<uintptr_t>(ws_dev) & 7)
    return fail(nullptr, XV_ERR_INVALID, "xv_metric_loss_grad: the workspace must be 8-byte aligned (it holds offsets and doubles)");
  return with_device(device, "xv_metric_loss_grad", [&] {
    return launch_metric_loss_grad(x_dev, ldx, offsets_host, num_groups, d, labels_dev, kind, pos_head, margin, squared ? 1 : 0,
                                   normalize ? 1 : 0, grad_scale, row_loss_dev, row_count_dev, group_loss_dev, group_count_dev,
                                   grad_x_dev, ldg, ws_dev, ws_bytes, to_stream(stream));
  });
}

}  // extern "C"
