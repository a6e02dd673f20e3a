// wsovod::ScratchT (wsovod_amd/csrc/scratch.h) over a fake device API: a counting allocator, a settable "capturing" flag and
// a settable device number.  Built and run by tests/test_scratch_host.py; exit status 0 and "scratch ok" when every check
// holds, else the failed checks on stderr.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../wsovod_amd/csrc/scratch.h"

namespace {

struct Fake {
  typedef int stream_t;
  static std::vector<size_t> sizes;  // bytes of every allocation, in order
  static std::vector<void*> blocks;
  static int frees;  // (the API has no free: the count, and the tag each block still carries, show that none happened)
  static constexpr char kAlive = 0x5a;
  static bool all_alive() {
    for (void* p : blocks)
      if (*(char*)p != kAlive) return false;
    return true;
  }
  static bool is_capturing, fail_next;
  static int dev;
  static void* alloc(size_t bytes) {
    if (fail_next) {
      fail_next = false;
      return nullptr;
    }
    char* p = (char*)malloc(1);  // the size is bookkeeping only: no request here touches that much memory
    *p = kAlive;
    sizes.push_back(bytes);
    blocks.push_back(p);
    return p;
  }
  static bool capturing(int) { return is_capturing; }
  static int device() { return dev; }
  static void reset() {
    for (void* p : blocks) free(p);  // the test's own cleanup between rules, outside the counted API
    sizes.clear();
    blocks.clear();
    frees = 0;
    is_capturing = fail_next = false;
    dev = 0;
  }
};
std::vector<size_t> Fake::sizes;
std::vector<void*> Fake::blocks;
int Fake::frees = 0;
bool Fake::is_capturing = false, Fake::fail_next = false;
int Fake::dev = 0;

using wsovod::ScratchGrowth;
using wsovod::ScratchStatus;
typedef wsovod::ScratchT<Fake> Scratch;

int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, rule, #cond); \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

// What holds under every rule.  first / larger: two requests, the second beyond what the first allocation holds;
// want_first / want_larger: the sizes the rule must allocate for them (want_larger 0: the rule refuses to grow)
void common(const char* rule, ScratchGrowth growth, size_t first, size_t want_first, size_t larger, size_t want_larger) {
  Fake::reset();
  Scratch ws(growth);
  ScratchStatus st;
  void* a = ws.reserve(first, 0, &st);
  CHECK(a && st == ScratchStatus::ok);
  CHECK(Fake::sizes.size() == 1 && Fake::sizes[0] == want_first);
  // a request that fits returns the same pointer, also one of exactly the live size
  CHECK(ws.reserve(first, 0, &st) == a && st == ScratchStatus::ok);
  CHECK(ws.reserve(1, 0, &st) == a && st == ScratchStatus::ok);
  CHECK(ws.reserve(want_first, 0, &st) == a && st == ScratchStatus::ok);
  CHECK(Fake::sizes.size() == 1);
  // growth under capture: refused, nothing allocated; a request that fits is served while capturing
  Fake::is_capturing = true;
  CHECK(ws.reserve(larger, 0, &st) == nullptr && st == ScratchStatus::would_grow_under_capture);
  CHECK(Fake::sizes.size() == 1);
  CHECK(ws.reserve(first, 0, &st) == a && st == ScratchStatus::ok);
  Fake::is_capturing = false;
  // a failed allocation leaves the live block in place
  Fake::fail_next = true;
  CHECK(ws.reserve(larger, 0, &st) == nullptr && st == ScratchStatus::alloc_failed);
  Fake::fail_next = false;
  CHECK(Fake::sizes.size() == 1);
  CHECK(ws.reserve(first, 0, &st) == a && st == ScratchStatus::ok);
  // a larger request: a new pointer, the old block still allocated
  void* b = ws.reserve(larger, 0, &st);
  if (want_larger) {
    CHECK(b && b != a && st == ScratchStatus::ok);
    CHECK(Fake::sizes.size() == 2 && Fake::sizes[1] == want_larger);
    CHECK(ws.reserve(first, 0, &st) == b);
  } else {
    CHECK(b == nullptr && st == ScratchStatus::alloc_failed);
    CHECK(Fake::sizes.size() == 1);
    CHECK(ws.reserve(first, 0, &st) == a);
  }
  CHECK(Fake::frees == 0);
  // device 1 gets a block of its own, under the rule's first-use size; device 0's is unchanged
  void* live0 = ws.reserve(first, 0, &st);
  const size_t n = Fake::sizes.size();
  Fake::dev = 1;
  Fake::is_capturing = true;  // (its first use is growth as well)
  CHECK(ws.reserve(first, 0, &st) == nullptr && st == ScratchStatus::would_grow_under_capture);
  Fake::is_capturing = false;
  void* c = ws.reserve(first, 0, &st);
  CHECK(c && c != a && c != b && st == ScratchStatus::ok);
  CHECK(Fake::sizes.size() == n + 1 && Fake::sizes[n] == want_first);
  CHECK(ws.reserve(first, 0, &st) == c);
  Fake::dev = 0;
  CHECK(ws.reserve(first, 0, &st) == live0);
  CHECK(Fake::sizes.size() == n + 1 && Fake::frees == 0 && Fake::all_alive());
}

}  // namespace

int main() {
  const size_t MB = (size_t)1 << 20;
  {
    const char* rule = "doubling";
    common(rule, ScratchGrowth::doubling(), 100, 100, 101, 200);  // max(need, 2 * have): doubling wins
    common(rule, ScratchGrowth::doubling(), 100, 100, 1000, 1000);  // the request wins
    Fake::reset();
    Scratch ws(ScratchGrowth::doubling());
    ScratchStatus st;
    const size_t asks[] = {3 * MB, 4 * MB, 7 * MB, 8 * MB, 100 * MB, 150 * MB};
    const size_t want[] = {3 * MB, 6 * MB, 12 * MB, 100 * MB, 200 * MB};  // (8 MB fits the 12 MB block)
    for (size_t r : asks) CHECK(ws.reserve(r, 0, &st) != nullptr && st == ScratchStatus::ok);
    CHECK(Fake::sizes.size() == 5);
    for (size_t i = 0; i < Fake::sizes.size() && i < 5; ++i) CHECK(Fake::sizes[i] == want[i]);
    // retired blocks together stay smaller than the live one
    size_t retired = 0;
    for (size_t i = 0; i + 1 < Fake::sizes.size(); ++i) retired += Fake::sizes[i];
    CHECK(retired < Fake::sizes.back());
    CHECK(Fake::frees == 0);
  }
  {
    const char* rule = "doubling_capped";
    const size_t cap = (size_t)128 * 65536 * 4;  // the fused-SGD tail scratch: 32 MB
    const size_t tile = (size_t)65536 * 4;
    common(rule, ScratchGrowth::doubling_capped(cap), 100, 100, 101, 200);
    common(rule, ScratchGrowth::doubling_capped(cap), 10 * tile, 10 * tile, 11 * tile, 20 * tile);
    common(rule, ScratchGrowth::doubling_capped(cap), 100 * tile, 100 * tile, 101 * tile, cap);  // min(2 * have, cap) = cap
    common(rule, ScratchGrowth::doubling_capped(cap), cap, cap, cap + 1, cap + 1);  // at the cap: the request alone
    Fake::reset();
    Scratch ws(ScratchGrowth::doubling_capped(cap));
    ScratchStatus st;
    const size_t asks[] = {40 * tile, 70 * tile, 90 * tile, 128 * tile};
    const size_t want[] = {40 * tile, 80 * tile, 128 * tile};  // (128 tiles fit the block allocated for 90)
    for (size_t r : asks) CHECK(ws.reserve(r, 0, &st) != nullptr && st == ScratchStatus::ok);
    CHECK(Fake::sizes.size() == 3);
    for (size_t i = 0; i < Fake::sizes.size() && i < 3; ++i) CHECK(Fake::sizes[i] == want[i]);
    CHECK(Fake::frees == 0);
  }
  {
    const char* rule = "fixed_size";
    // ONE allocation of the fixed size whatever is asked first; never replaced: a larger request fails, the block stays
    common(rule, ScratchGrowth::fixed_size(64 * MB), 100, 64 * MB, 64 * MB + 1, 0);
    common(rule, ScratchGrowth::fixed_size(2048), 2048, 2048, 4096, 0);
    Fake::reset();
    Scratch ws(ScratchGrowth::fixed_size(2048));
    ScratchStatus st;
    CHECK(ws.reserve(4096, 0, &st) == nullptr && st == ScratchStatus::alloc_failed);  // larger than the block can ever be
    CHECK(Fake::sizes.empty());
    void* a = ws.reserve(8, 0, &st);
    for (size_t r = 1; r <= 2048; r *= 2) CHECK(ws.reserve(r, 0, &st) == a && st == ScratchStatus::ok);
    CHECK(Fake::sizes.size() == 1 && Fake::sizes[0] == 2048 && Fake::frees == 0);
  }
  {
    const char* rule = "devices";
    Fake::reset();
    Scratch ws(ScratchGrowth::doubling());
    ScratchStatus st;
    Fake::dev = 3;  // first use on a device that is not the first
    void* d3 = ws.reserve(64, 0, &st);
    CHECK(d3 && st == ScratchStatus::ok);
    Fake::dev = 0;
    void* d0 = ws.reserve(32, 0, &st);
    CHECK(d0 && d0 != d3 && Fake::sizes.size() == 2 && Fake::sizes[1] == 32);
    void* d0b = ws.reserve(48, 0, &st);  // device 0 grows: 64 bytes; device 3's block does not move
    CHECK(d0b && d0b != d0 && Fake::sizes.size() == 3 && Fake::sizes[2] == 64);
    Fake::dev = 3;
    CHECK(ws.reserve(64, 0, &st) == d3);
    CHECK(Fake::sizes.size() == 3 && Fake::frees == 0);
  }
  Fake::reset();
  if (failures) {
    fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  printf("scratch ok\n");
  return 0;
}
