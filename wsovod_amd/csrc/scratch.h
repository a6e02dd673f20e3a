// The grow-only device workspace of the library, written once (no HIP in this header: the device API is a policy, so the
// growth logic runs on the host alone in tests/host/scratch_main.cpp).
//
// A captured HIP graph keeps the pointer it was captured with, so a block is NEVER freed once handed out: when a larger one
// is needed the old block is retired (kept allocated) and a fresh one becomes the live block, and growing under stream
// capture is refused instead of allocating inside the capture -- what the caller does then (an error, a single launch, a
// kernel path without workspace) is the caller's.  Blocks are kept per device: the live block and the retired ones of the
// device that is current at the call.  Single-stream use, as the rest of the library: nothing here locks.
//
// Api:  typedef ... stream_t;
//       static void* alloc(size_t bytes);        nullptr on failure, with the API's sticky error cleared
//       static bool capturing(stream_t stream);
//       static int device();                     the current device, >= 0
#pragma once
#include <stddef.h>

#include <algorithm>
#include <vector>

namespace wsovod {

enum class ScratchStatus { ok, would_grow_under_capture, alloc_failed };

// How a block that is too small is replaced.  With `have` the live size and `need` the request:
struct ScratchGrowth {
  size_t cap;    // the new size is max(need, min(2 * have, cap))
  size_t fixed;  // != 0: ONE block of this size at first use, never replaced (a larger request fails)
  static ScratchGrowth doubling() { return {(size_t)-1, 0}; }  // retired blocks together stay smaller than the live one
  static ScratchGrowth doubling_capped(size_t cap) { return {cap, 0}; }
  static ScratchGrowth fixed_size(size_t bytes) { return {0, bytes}; }
};

template <class Api>
class ScratchT {
 public:
  explicit ScratchT(ScratchGrowth growth) : growth_(growth) {}

  // a block of at least `bytes` on the current device, or nullptr (*status says why)
  void* reserve(size_t bytes, typename Api::stream_t stream, ScratchStatus* status) {
    const int dev = std::max(0, Api::device());
    if ((size_t)dev >= per_device_.size()) per_device_.resize(dev + 1);
    Blocks& b = per_device_[dev];
    *status = ScratchStatus::ok;
    if (bytes <= b.live_bytes) return b.live;
    if (Api::capturing(stream)) {
      *status = ScratchStatus::would_grow_under_capture;
      return nullptr;
    }
    const size_t doubled = b.live_bytes > growth_.cap / 2 ? growth_.cap : 2 * b.live_bytes;
    const size_t want = growth_.fixed ? growth_.fixed : std::max(bytes, doubled);
    void* fresh = (growth_.fixed && (b.live || bytes > growth_.fixed)) ? nullptr : Api::alloc(want);
    if (!fresh) {
      *status = ScratchStatus::alloc_failed;
      return nullptr;
    }
    if (b.live) b.retired.push_back(b.live);
    b.live = fresh;
    b.live_bytes = want;
    return fresh;
  }

 private:
  struct Blocks {
    void* live = nullptr;
    size_t live_bytes = 0;
    std::vector<void*> retired;  // never freed
  };
  ScratchGrowth growth_;
  std::vector<Blocks> per_device_;
};

}  // namespace wsovod
