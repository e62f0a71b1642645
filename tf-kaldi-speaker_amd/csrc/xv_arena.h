// Workspace arena of the batch planner (api_plan.hip): byte offsets into one buffer, first fit, release after last use.
// Plain C++17, no HIP: tests/host/arena_check.cpp drives it on the host under ASan / UBSan.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace xv {

class Arena {
 public:
  struct Block { int64_t off, size; };

  // First free block that is large enough, carved from its front; otherwise the arena grows at the top.
  int64_t alloc(int64_t size) {
    for (size_t i = 0; i < free_.size(); ++i)
      if (free_[i].size >= size) {
        const int64_t off = free_[i].off;
        free_[i].off += size;
        free_[i].size -= size;
        if (free_[i].size == 0) free_.erase(free_.begin() + i);
        return off;
      }
    const int64_t off = top_;
    top_ += size;
    return off;
  }

  // The free list stays sorted by offset, and a block is merged with the neighbours it touches.
  void release(int64_t off, int64_t size) {
    auto it = std::upper_bound(free_.begin(), free_.end(), off, [](int64_t o, const Block& b) { return o < b.off; });
    it = free_.insert(it, Block{off, size});
    if (it + 1 != free_.end() && it->off + it->size == (it + 1)->off) {
      it->size += (it + 1)->size;
      it = free_.erase(it + 1) - 1;
    }
    if (it != free_.begin() && (it - 1)->off + (it - 1)->size == it->off) {
      (it - 1)->size += it->size;
      free_.erase(it);
    }
  }

  int64_t top() const { return top_; }                       // bytes the workspace needs
  const std::vector<Block>& free_list() const { return free_; }

 private:
  std::vector<Block> free_;
  int64_t top_ = 0;
};

}  // namespace xv
