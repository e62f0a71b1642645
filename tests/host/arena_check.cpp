// Host check of the planner's workspace arena (tf-kaldi-speaker_amd/csrc/xv_arena.h), built with -fsanitize=address,undefined
// by tests/test_arena_host.py.  Three fixed sequences with hand-written offsets, then seeded random alloc / release
// sequences (sizes are multiples of 256, as in the planner) with every invariant checked after every call.
#include <stdint.h>

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "xv_arena.h"

using xv::Arena;

namespace {

struct Live { int64_t off, size; };

#define CHECK(cond)                                                                    \
  do {                                                                                 \
    if (!(cond)) {                                                                     \
      std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond);    \
      std::exit(1);                                                                    \
    }                                                                                  \
  } while (0)

bool overlap(int64_t a, int64_t an, int64_t b, int64_t bn) { return a < b + bn && b < a + an; }

void check_invariants(const Arena& ar, const std::vector<Live>& live) {
  const auto& fl = ar.free_list();
  for (size_t i = 0; i < live.size(); ++i) {
    CHECK(live[i].off >= 0 && live[i].off + live[i].size <= ar.top());           // every live block lies below top()
    for (size_t j = i + 1; j < live.size(); ++j)                                 // no two live blocks overlap
      CHECK(!overlap(live[i].off, live[i].size, live[j].off, live[j].size));
    for (const auto& f : fl) CHECK(!overlap(live[i].off, live[i].size, f.off, f.size));   // free list disjoint from the live blocks
  }
  int64_t bytes = 0;
  for (size_t i = 0; i < fl.size(); ++i) {
    CHECK(fl[i].size > 0 && fl[i].off >= 0 && fl[i].off + fl[i].size <= ar.top());
    if (i + 1 < fl.size()) CHECK(fl[i].off + fl[i].size < fl[i + 1].off);        // sorted, and never adjacent (merged)
    bytes += fl[i].size;
  }
  for (const Live& l : live) bytes += l.size;
  CHECK(bytes == ar.top());                                                      // nothing leaks: live + free = [0, top())
}

void fixed_sequences() {
  {   // reuse of an exact-fit hole
    Arena a;
    CHECK(a.alloc(256) == 0);
    CHECK(a.alloc(512) == 256);
    CHECK(a.alloc(256) == 768);
    a.release(256, 512);
    CHECK(a.free_list().size() == 1 && a.free_list()[0].off == 256 && a.free_list()[0].size == 512);
    CHECK(a.alloc(512) == 256);
    CHECK(a.free_list().empty() && a.top() == 1024);
    CHECK(a.alloc(256) == 1024 && a.top() == 1280);
  }
  {   // a split from the front: the rest of the hole stays free, and first fit skips a hole that is too small
    Arena a;
    CHECK(a.alloc(256) == 0);
    CHECK(a.alloc(256) == 256);
    CHECK(a.alloc(1024) == 512);
    CHECK(a.alloc(256) == 1536);
    a.release(0, 256);
    a.release(512, 1024);
    CHECK(a.alloc(512) == 512);            // hole [0, 256) is too small
    CHECK(a.free_list().size() == 2 && a.free_list()[1].off == 1024 && a.free_list()[1].size == 512);
    CHECK(a.alloc(256) == 0);              // first fit: the lowest hole that is large enough
    CHECK(a.alloc(256) == 1024);
    CHECK(a.alloc(256) == 1280);
    CHECK(a.free_list().empty() && a.top() == 1792);
  }
  {   // a three-way merge: the middle block goes back last
    Arena a;
    CHECK(a.alloc(256) == 0);
    CHECK(a.alloc(512) == 256);
    CHECK(a.alloc(768) == 768);
    CHECK(a.alloc(256) == 1536);
    a.release(768, 768);
    a.release(0, 256);
    CHECK(a.free_list().size() == 2);
    a.release(256, 512);
    CHECK(a.free_list().size() == 1 && a.free_list()[0].off == 0 && a.free_list()[0].size == 1536);
    CHECK(a.alloc(1536) == 0);
    CHECK(a.free_list().empty() && a.top() == 1792);
  }
}

void random_sequence(unsigned seed, int calls) {
  std::mt19937 rng(seed);
  Arena ar;
  std::vector<Live> live;
  for (int i = 0; i < calls; ++i) {
    const bool do_alloc = live.empty() || rng() % 100 < 55;
    if (do_alloc) {
      const int64_t size = 256 * (int64_t)(1 + rng() % (rng() % 4 == 0 ? 4096 : 16));
      const int64_t top0 = ar.top();
      const int64_t off = ar.alloc(size);
      CHECK(off % 256 == 0);
      CHECK(ar.top() == top0 || (off == top0 && ar.top() == top0 + size));       // grows only when it allocates at the top
      live.push_back({off, size});
    } else {
      const size_t k = rng() % live.size();
      ar.release(live[k].off, live[k].size);
      live.erase(live.begin() + k);
    }
    check_invariants(ar, live);
  }
  while (!live.empty()) {
    const size_t k = rng() % live.size();
    ar.release(live[k].off, live[k].size);
    live.erase(live.begin() + k);
    check_invariants(ar, live);
  }
  // releasing everything leaves exactly one free block [0, top())
  CHECK(ar.top() == 0 ? ar.free_list().empty()
                      : ar.free_list().size() == 1 && ar.free_list()[0].off == 0 && ar.free_list()[0].size == ar.top());
}

}  // namespace

int main() {
  fixed_sequences();
  for (unsigned seed = 1; seed <= 40; ++seed) random_sequence(seed, 400);
  std::printf("arena ok\n");
  return 0;
}
