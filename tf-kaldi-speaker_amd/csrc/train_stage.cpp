// The stager of training input: copy the bytes a planned batch needs, and nothing else, from the archives into one
// caller-provided (pinned) buffer and describe them for xv_train_batch_decode (csrc/train_batch.hip).  The rule is in
// include/xvec_hip.h (xv_train_stage).  Record headers are read as csrc/ark_io.cpp reads them:
//   [key SP] \0 B  'FM '|'DM '  \4 <i32 rows> \4 <i32 cols> payload                       (row-major floats / doubles)
//   [key SP] \0 B  'CM '  <f32 min><f32 range><i32 rows><i32 cols>  cols x 4 x u16, column-major u8 payload
// A chunk of an 'FM ' / 'DM ' record is one contiguous range of the file; a chunk of a 'CM ' record is the cols x 8 header bytes
// and `length` bytes out of every column.  The threads only pread: no arithmetic touches a feature value on the host.
// Plain C ABI, no HIP calls: usable and tested without a GPU.  Every failure is a status and a message, never a crash: all
// sizes come from the file and are checked against its length before a byte is copied.
#include <errno.h>
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../../include/xvec_hip.h"

namespace {

struct Source {                 // where the bytes of one chunk lie in its file
  int fd = -1;
  int64_t headers = 0;          // CM: file offset of the column headers
  int64_t data = 0;             // file offset of element (0, 0) of the payload
  int32_t file_rows = 0;        // rows of the whole record (the column stride of a CM payload in the file)
  int64_t bytes = 0;            // staged bytes of the chunk, its padding to 16 not counted
};

bool pread_all(int fd, void* dst, size_t n, int64_t off) {
  unsigned char* out = static_cast<unsigned char*>(dst);
  while (n > 0) {
    const ssize_t got = pread(fd, out, n, (off_t)off);
    if (got < 0 && errno == EINTR) continue;
    if (got <= 0) return false;
    out += got;
    off += got;
    n -= (size_t)got;
  }
  return true;
}

int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// header of the record at `offset` of fd (file_size bytes long) -> c (kind, cols, gmin, grange) and s; "" or the complaint
std::string parse_record(int fd, int64_t file_size, int64_t offset, int start, int length, xv_train_chunk* c, Source* s) {
  unsigned char h[320];
  if (offset < 0 || offset >= file_size) return "offset beyond the end of the file";
  const size_t have = (size_t)(file_size - offset < (int64_t)sizeof(h) ? file_size - offset : (int64_t)sizeof(h));
  if (!pread_all(fd, h, have, offset)) return std::string("read failed: ") + strerror(errno);
  size_t p = 0;
  if (have >= 1 && h[0] != 0) {                         // a key in front of the record: skip it
    const void* sp = memchr(h, ' ', have < 257 ? have : 257);
    if (!sp) return "neither \\0B nor a key of at most 256 bytes at the offset";
    p = (size_t)(static_cast<const unsigned char*>(sp) - h) + 1;
  }
  if (have < p + 5) return "truncated file: the record header is cut off";
  if (h[p] != 0 || h[p + 1] != 'B') return "text-mode or unknown record (expected \\0B)";
  int kind = 0;
  if (!memcmp(h + p + 2, "FM ", 3)) kind = XV_TRAIN_FM;
  else if (!memcmp(h + p + 2, "DM ", 3)) kind = XV_TRAIN_DM;
  else if (!memcmp(h + p + 2, "CM ", 3)) kind = XV_TRAIN_CM;
  else return "unknown kind (FM / DM / CM records are staged)";
  p += 5;
  int32_t rows = 0, cols = 0;
  float gmin = 0.f, grange = 0.f;
  if (kind == XV_TRAIN_CM) {
    if (have < p + 16) return "truncated file: the compressed-matrix header is cut off";
    memcpy(&gmin, h + p, 4);
    memcpy(&grange, h + p + 4, 4);
    memcpy(&rows, h + p + 8, 4);
    memcpy(&cols, h + p + 12, 4);
    p += 16;
  } else {
    if (have < p + 10) return "truncated file: the matrix header is cut off";
    if (h[p] != 4 || h[p + 5] != 4) return "matrix header: int-size markers missing";
    memcpy(&rows, h + p + 1, 4);
    memcpy(&cols, h + p + 6, 4);
    p += 10;
  }
  if (rows < 0 || cols < 0) return "negative matrix dimension";
  if (cols < 1) return "a record without columns";
  if ((int64_t)start + length > rows) {
    char msg[128];
    snprintf(msg, sizeof(msg), "short record: %d rows, the chunk needs rows [%d, %lld)", rows, start, (long long)start + length);
    return msg;
  }
  const int64_t es = kind == XV_TRAIN_FM ? 4 : (kind == XV_TRAIN_DM ? 8 : 1);
  const int64_t body = offset + (int64_t)p;
  const int64_t cells = (int64_t)rows * cols;                            // below 2^62: both are int32
  if (cells > ((int64_t)1 << 56) || (kind == XV_TRAIN_CM ? (int64_t)cols * 8 : 0) + cells * es > file_size - body)
    return "truncated file: the payload is cut off";
  c->kind = kind;
  c->cols = cols;
  c->rows = length;
  c->first_row = 0;
  c->gmin = gmin;
  c->grange = grange;
  s->fd = fd;
  s->file_rows = rows;
  if (kind == XV_TRAIN_CM) {
    s->headers = body;
    s->data = body + (int64_t)cols * 8 + start;
    s->bytes = align16((int64_t)cols * 8) + (int64_t)cols * length;
  } else {
    s->data = body + (int64_t)start * cols * es;
    s->bytes = (int64_t)length * cols * es;
  }
  return "";
}

bool copy_chunk(const xv_train_chunk& c, const Source& s, unsigned char* dst) {
  if (c.kind != XV_TRAIN_CM) return pread_all(s.fd, dst + c.payload_off, (size_t)s.bytes, s.data);
  if (!pread_all(s.fd, dst + c.header_off, (size_t)c.cols * 8, s.headers)) return false;
  for (int64_t col = 0; col < c.cols; ++col)
    if (!pread_all(s.fd, dst + c.payload_off + col * c.rows, (size_t)c.rows, s.data + col * s.file_rows)) return false;
  return true;
}

}  // namespace

extern "C" int xv_train_stage(const char* rxfiles, int n, const int32_t* starts, int length, int threads, void* dst,
                              int64_t dst_capacity, xv_train_chunk* chunks, int32_t* status, int64_t* staged_bytes, char* err,
                              int64_t err_capacity) {
  if (err && err_capacity > 0) err[0] = 0;
  if (!rxfiles || !starts || !dst || !chunks || !status || !staged_bytes || n < 1 || length < 1 || dst_capacity < 0)
    return XV_ERR_INVALID;
  *staged_bytes = 0;
  std::string first_error;
  auto complain = [&](int i, int code, const std::string& rx, const std::string& msg) {
    status[i] = code;
    memset(&chunks[i], 0, sizeof(chunks[i]));
    if (first_error.empty()) first_error = "chunk " + std::to_string(i) + " (" + rx + "): " + msg;
  };
  // 1. the headers, in chunk order: files are opened once per call and closed at its end
  std::vector<std::string> paths;
  std::vector<int> fds;
  std::vector<int64_t> sizes;
  std::vector<Source> src((size_t)n);
  const char* line = rxfiles;
  int failed = 0;
  for (int i = 0; i < n; ++i) {
    const char* e = strchr(line, '\n');
    if (!e) {
      for (int fd : fds) if (fd >= 0) close(fd);
      return XV_ERR_INVALID;                              // fewer than n rxfilenames
    }
    std::string rx(line, e - line);
    line = e + 1;
    status[i] = XV_OK;
    while (!rx.empty() && (rx.back() == ' ' || rx.back() == '\t' || rx.back() == '\r')) rx.pop_back();
    if (starts[i] < 0) { complain(i, XV_ERR_INVALID, rx, "negative start"); ++failed; continue; }
    if (rx.empty() || rx.back() == '|' || rx.back() == ']' || rx[0] == '|') {
      complain(i, XV_ERR_UNSUPPORTED, rx, "a pipe or a range as rxfilename is not staged natively");
      ++failed;
      continue;
    }
    int64_t offset = 0;
    std::string path = rx;
    const size_t colon = rx.rfind(':');
    if (colon != std::string::npos && colon + 1 < rx.size() && rx.size() - colon <= 19 &&
        rx.find_first_not_of("0123456789", colon + 1) == std::string::npos) {
      offset = strtoll(rx.c_str() + colon + 1, nullptr, 10);
      path.erase(colon);
    }
    int pi = -1;
    for (size_t k = paths.size(); k-- > 0;) if (paths[k] == path) { pi = (int)k; break; }
    if (pi < 0) {
      const int fd = open(path.c_str(), O_RDONLY);
      struct stat st;
      int64_t size = -1;
      if (fd >= 0 && fstat(fd, &st) == 0 && S_ISREG(st.st_mode)) size = (int64_t)st.st_size;
      paths.push_back(path);
      fds.push_back(fd);
      sizes.push_back(size);
      pi = (int)paths.size() - 1;
    }
    if (fds[pi] < 0) { complain(i, XV_ERR_INVALID, rx, "cannot open the file"); ++failed; continue; }
    if (sizes[pi] < 0) { complain(i, XV_ERR_INVALID, rx, "not a regular file"); ++failed; continue; }
    const std::string msg = parse_record(fds[pi], sizes[pi], offset, starts[i], length, &chunks[i], &src[i]);
    if (!msg.empty()) { complain(i, XV_ERR_INVALID, rx, msg); ++failed; }
  }
  // 2. the layout: chunk order, 16-byte boundaries, a function of the records alone
  int64_t total = 0;
  for (int i = 0; i < n; ++i) {
    if (status[i] != XV_OK) continue;
    if (chunks[i].kind == XV_TRAIN_CM) {
      chunks[i].header_off = total;
      chunks[i].payload_off = total + align16((int64_t)chunks[i].cols * 8);
    } else {
      chunks[i].header_off = 0;
      chunks[i].payload_off = total;
    }
    total = align16(total + src[i].bytes);
  }
  *staged_bytes = total;
  int rc = failed;
  if (total > dst_capacity) {
    rc = XV_ERR_WORKSPACE;
    if (first_error.empty()) first_error = "the staging buffer holds " + std::to_string(dst_capacity) + " bytes, the batch needs " + std::to_string(total);
  } else {
    // 3. the copies: chunks are dealt out one at a time; every chunk writes its own bytes, so the result does not depend on who copies
    unsigned char* out = static_cast<unsigned char*>(dst);
    std::atomic<int> next{0};
    std::atomic<int> bad{-1};
    auto work = [&] {
      for (;;) {
        const int i = next.fetch_add(1, std::memory_order_relaxed);
        if (i >= n) return;
        if (status[i] != XV_OK) continue;
        if (!copy_chunk(chunks[i], src[i], out)) {
          int want = -1;
          bad.compare_exchange_strong(want, i);
        }
      }
    };
    int nt = threads < 1 ? 1 : (threads > 16 ? 16 : threads);
    if (nt > n) nt = n;
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back(work);
    work();
    for (auto& x : th) x.join();
    if (bad.load() >= 0) {                               // the file shrank under the call: headers promised bytes that are gone
      rc = XV_ERR_INVALID;
      first_error = "chunk " + std::to_string(bad.load()) + ": pread failed inside the payload (truncated file)";
    }
  }
  for (int fd : fds) if (fd >= 0) close(fd);
  if (err && err_capacity > 0) {
    const size_t m = first_error.size() < (size_t)err_capacity - 1 ? first_error.size() : (size_t)err_capacity - 1;
    memcpy(err, first_error.data(), m);
    err[m] = 0;
  }
  return rc;
}
