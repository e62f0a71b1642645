// Stand-alone check of the training-input stager for sanitizer builds (no GPU, no Python):
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tests/host/train_stage_check.cpp \
//       tf-kaldi-speaker_amd/csrc/train_stage.cpp tf-kaldi-speaker_amd/csrc/ark_io.cpp -lpthread -o train_stage_check
//   ./train_stage_check <scratch directory>
// It writes 'FM ', 'DM ' and 'CM ' archives itself (cols 1, 3, 30, 33; rows 1, 64, 65, 300; any bytes are a valid 'CM ' payload),
// stages chunks at start 0, at rows - length and of the whole record with 1 and 16 threads, decodes the staged bytes by the rule
// of include/xvec_hip.h and compares every element's bits with what xv_ark_next_batch decodes for the record; then the refused
// inputs: a truncated file (cut in the payload, in the header, before the record), an unknown kind, a short record, a pipe, a
// range, a missing file, too small a buffer, bad arguments.  Prints "ok" and returns 0, or the first difference and 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "xvec_hip.h"

namespace {

uint32_t rng_state = 12345u;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

void put(std::vector<unsigned char>& out, const void* p, size_t n) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  out.insert(out.end(), b, b + n);
}

// one record behind "key ": returns the offset of its "\0B"
int64_t add_record(std::vector<unsigned char>& file, const std::string& key, int kind, int32_t rows, int32_t cols) {
  put(file, key.data(), key.size());
  file.push_back(' ');
  const int64_t at = (int64_t)file.size();
  const char* tag = kind == XV_TRAIN_FM ? "FM " : (kind == XV_TRAIN_DM ? "DM " : "CM ");
  file.push_back(0);
  file.push_back('B');
  put(file, tag, 3);
  if (kind == XV_TRAIN_CM) {
    const float gmin = -7.25f, grange = 19.5f;
    put(file, &gmin, 4);
    put(file, &grange, 4);
    put(file, &rows, 4);
    put(file, &cols, 4);
    for (int64_t i = 0; i < (int64_t)cols * 4; ++i) { const uint16_t h = (uint16_t)rnd(); put(file, &h, 2); }
    for (int64_t i = 0; i < (int64_t)cols * rows; ++i) file.push_back((unsigned char)rnd());
  } else {
    file.push_back(4);
    put(file, &rows, 4);
    file.push_back(4);
    put(file, &cols, 4);
    for (int64_t i = 0; i < (int64_t)cols * rows; ++i) {
      const double v = ((double)rnd() / (1 << 23) - 1.0) * 3.0 + (double)rnd() * 1e-12;
      if (kind == XV_TRAIN_FM) { const float f = (float)v; put(file, &f, 4); } else put(file, &v, 8);
    }
  }
  return at;
}

bool write_file(const std::string& path, const std::vector<unsigned char>& bytes, size_t keep) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = fwrite(bytes.data(), 1, keep, f) == keep;
  return fclose(f) == 0 && ok;
}

// the rule of include/xvec_hip.h on the staged bytes -> element (t, c) of the chunk
float decode(const unsigned char* buf, const xv_train_chunk& d, int t, int c) {
  const int64_t r = d.first_row + t;
  if (d.kind == XV_TRAIN_FM) { float v; memcpy(&v, buf + d.payload_off + (r * d.cols + c) * 4, 4); return v; }
  if (d.kind == XV_TRAIN_DM) { double v; memcpy(&v, buf + d.payload_off + (r * d.cols + c) * 8, 8); return (float)v; }
  uint16_t h[4];
  memcpy(h, buf + d.header_off + 8 * (int64_t)c, 8);
  double p[4];
  for (int i = 0; i < 4; ++i) p[i] = (double)(float)((double)d.gmin + (double)d.grange * 1.52590218966964e-05 * h[i]);
  const int v = buf[d.payload_off + (int64_t)c * d.rows + r];
  double x;
  if (v <= 64) x = p[0] + (p[1] - p[0]) / 64. * v;
  else if (v <= 192) x = p[1] + (p[2] - p[1]) / 128. * (v - 64);
  else x = p[2] + (p[3] - p[2]) / 63. * (v - 192);
  return (float)x;
}

int fails = 0;
#define EXPECT(cond, ...)                                                                     \
  do {                                                                                        \
    if (!(cond)) { printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); ++fails; } \
  } while (0)

struct Staged {
  int rc;
  std::vector<xv_train_chunk> chunks;
  std::vector<int32_t> status;
  int64_t bytes = 0;
  std::string err;
};

Staged stage(const std::string& rx, const std::vector<int32_t>& starts, int length, int threads, std::vector<unsigned char>& dst) {
  Staged s;
  const int n = (int)starts.size();
  s.chunks.resize(n);
  s.status.assign(n, 77);
  char err[512];
  s.rc = xv_train_stage(rx.c_str(), n, starts.data(), length, threads, dst.data(), (int64_t)dst.size(), s.chunks.data(), s.status.data(),
                        &s.bytes, err, sizeof(err));
  s.err = err;
  return s;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  const int kinds[3] = {XV_TRAIN_FM, XV_TRAIN_DM, XV_TRAIN_CM};
  const int32_t colses[4] = {1, 3, 30, 33}, rowses[4] = {1, 64, 65, 300};
  for (int kind : kinds) {
    std::vector<unsigned char> file;
    struct Rec { int64_t at; int32_t rows, cols; };
    std::vector<Rec> recs;
    for (int32_t cols : colses)
      for (int32_t rows : rowses) recs.push_back({add_record(file, "utt" + std::to_string(recs.size()), kind, rows, cols), rows, cols});
    const std::string path = dir + "/stage_" + std::to_string(kind) + ".ark";
    if (!write_file(path, file, file.size())) { printf("cannot write %s\n", path.c_str()); return 2; }
    // the oracle: every record through the native reader
    xv_ark_reader* r = nullptr;
    EXPECT(xv_ark_open(path.c_str(), -1, &r) == XV_OK, "open");
    std::vector<std::vector<float>> want;
    for (const Rec& rec : recs) {
      std::vector<float> m((size_t)rec.rows * rec.cols);
      int32_t offsets[2];
      char keys[64];
      int n = 0, dim = 0;
      const int rc = xv_ark_next_batch(r, 1, 1, 0, m.data(), (int64_t)m.size(), offsets, keys, sizeof(keys), &n, &dim);
      EXPECT(rc == 1 && dim == rec.cols && offsets[1] == rec.rows, "native reader: rc %d (%s)", rc, xv_ark_error(r));
      want.push_back(m);
    }
    xv_ark_close(r);
    std::vector<unsigned char> dst(1 << 20);
    for (size_t i = 0; i < recs.size(); ++i) {
      const Rec& rec = recs[i];
      const std::string rx = path + ":" + std::to_string(rec.at) + "\n";
      for (int length : {1, (rec.rows + 1) / 2, (int)rec.rows})
        for (int32_t start : {0, rec.rows - length})
          for (int threads : {1, 16}) {
            memset(dst.data(), 0xA5, dst.size());
            // the same record three times in one call: several chunks, several threads
            Staged s = stage(rx + rx + rx, {start, start, start}, length, threads, dst);
            EXPECT(s.rc == 0 && s.err.empty(), "kind %d record %zu: rc %d %s", kind, i, s.rc, s.err.c_str());
            if (s.rc != 0) continue;
            for (int k = 0; k < 3; ++k) {
              const xv_train_chunk& d = s.chunks[k];
              EXPECT(d.kind == kind && d.cols == rec.cols && d.rows == length && d.first_row == 0 && d.payload_off % 16 == 0, "descriptor");
              for (int t = 0; t < length; ++t)
                for (int c = 0; c < rec.cols; ++c) {
                  const float got = decode(dst.data(), d, t, c), ref = want[i][(size_t)(start + t) * rec.cols + c];
                  if (memcmp(&got, &ref, 4) != 0) { EXPECT(false, "kind %d record %zu element (%d, %d): %a, native %a", kind, i, t, c, got, ref); t = length; break; }
                }
            }
            EXPECT(dst[(size_t)s.bytes] == 0xA5, "a byte behind the layout was written");
          }
    }
    // truncated: in the payload, in the header, before the record
    const Rec& last = recs.back();
    const std::string cut = dir + "/cut_" + std::to_string(kind) + ".ark";
    const std::string rx = cut + ":" + std::to_string(last.at) + "\n";
    for (size_t keep : {file.size() - 1, (size_t)last.at + 7, (size_t)last.at, (size_t)1}) {
      if (!write_file(cut, file, keep)) return 2;
      Staged s = stage(rx, {0}, last.rows, 4, dst);
      EXPECT(s.rc == 1 && s.status[0] == XV_ERR_INVALID && s.chunks[0].kind == 0 && !s.err.empty(), "truncated at %zu: rc %d %s", keep, s.rc, s.err.c_str());
    }
    // a short record, too small a buffer
    Staged s = stage(path + ":" + std::to_string(recs[1].at) + "\n", {60}, 5, 1, dst);
    EXPECT(s.rc == 1 && s.status[0] == XV_ERR_INVALID && s.err.find("short record") != std::string::npos, "short: %s", s.err.c_str());
    std::vector<unsigned char> tiny(32, 0xA5);
    s = stage(path + ":" + std::to_string(last.at) + "\n", {0}, last.rows, 1, tiny);
    EXPECT(s.rc == XV_ERR_WORKSPACE && s.bytes > 32 && tiny[0] == 0xA5 && tiny[31] == 0xA5, "small buffer: rc %d", s.rc);
  }
  std::vector<unsigned char> dst(1 << 12);
  {   // an unknown kind, text, nothing at all
    std::vector<unsigned char> odd;
    put(odd, "u \0BCM2", 7);
    odd.resize(80, 0);
    if (!write_file(dir + "/odd.ark", odd, odd.size())) return 2;
    Staged s = stage(dir + "/odd.ark:2\n", {0}, 1, 1, dst);
    EXPECT(s.rc == 1 && s.err.find("unknown kind") != std::string::npos, "unknown kind: %s", s.err.c_str());
    s = stage(dir + "/odd.ark:0\n", {0}, 1, 1, dst);                       // the key in front is skipped
    EXPECT(s.rc == 1 && s.err.find("unknown kind") != std::string::npos, "key skipped: %s", s.err.c_str());
    s = stage(dir + "/odd.ark:9\n", {0}, 1, 1, dst);                       // zeros: no \0B, no key
    EXPECT(s.rc == 1 && s.status[0] == XV_ERR_INVALID, "zeros: %s", s.err.c_str());
    s = stage(dir + "/odd.ark:99999999999999999\n", {0}, 1, 1, dst);
    EXPECT(s.rc == 1 && s.status[0] == XV_ERR_INVALID, "far offset: %s", s.err.c_str());
  }
  Staged s = stage("copy-feats ark:a ark:- |\n" + dir + "/odd.ark:2[0:3]\n" + dir + "/missing.ark:5\n\n", {0, 0, 0, 0}, 1, 3, dst);
  EXPECT(s.rc == 4 && s.status[0] == XV_ERR_UNSUPPORTED && s.status[1] == XV_ERR_UNSUPPORTED && s.status[2] == XV_ERR_INVALID &&
             s.status[3] == XV_ERR_UNSUPPORTED && s.bytes == 0 && s.err.find("chunk 0 ") == 0, "pipes and ranges: rc %d %s", s.rc, s.err.c_str());
  s = stage("a\n", {-1}, 1, 1, dst);
  EXPECT(s.rc == 1 && s.status[0] == XV_ERR_INVALID, "negative start");
  s = stage("a", {0}, 1, 1, dst);
  EXPECT(s.rc == XV_ERR_INVALID, "fewer names than chunks");
  s = stage("a\n", {0}, 0, 1, dst);
  EXPECT(s.rc == XV_ERR_INVALID, "length 0");
  int64_t bytes = 0;
  EXPECT(xv_train_stage(nullptr, 1, nullptr, 1, 1, nullptr, 0, nullptr, nullptr, &bytes, nullptr, 0) == XV_ERR_INVALID, "null pointers");
  if (fails) { printf("%d check(s) failed\n", fails); return 1; }
  printf("ok\n");
  return 0;
}
