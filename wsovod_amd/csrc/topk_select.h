// Top-k of one row by radix select + LDS bitonic sort, for one workgroup of 256 threads: the machinery of the MRRP RPN's
// grouped top-k (proposals.hip: rpn_group_topk_kernel) and of the MIST candidate selection (mist.hip: mist_select_kernel).
// Order and equality are torch.sort's (descending, stable): every NaN is one value above +inf, -0.0 == +0.0, equal values by
// position ascending.
//   1. radix select of the k-th largest over order-preserving 32-bit keys, four 8-bit digits from the top; every wavefront
//      owns one contiguous quarter of the row and its own LDS histogram, the row is re-read (L2) on each pass
//   2. compaction into LDS: every key above the threshold, plus the first `ties` keys equal to it by position (the
//      per-wavefront counts of the last histogram give each quarter its base, so the walk needs no barrier)
//   3. bitonic sort of the <= 2048 (key, ~position) words in LDS
#pragma once
#include "common.h"

constexpr int kTopkMax = 2048;

// Order-preserving key of a score; never 0 (the lowest, -inf, is 0x007fffff): key 0 marks a position that is no candidate.
__device__ __forceinline__ unsigned int topk_key(float x) {
  if (x != x) return 0xffffffffu;          // every NaN: one value, above +inf
  if (x == 0.f) return 0x80000000u;        // -0.0 == +0.0
  const unsigned int u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct TopkShared {
  unsigned long long items[kTopkMax];  // (key << 32) | ~position: descending = key desc, position asc
  unsigned int hist[4][256];
  unsigned int sel[2];                 // digit chosen by the current pass, what remains of k below it
  unsigned int wave_eq[4];             // keys equal to the threshold in each wavefront's quarter
  unsigned int n_above;                // compaction cursor of the keys above the threshold
};

// key_at(p) -> the key of position p in [0, n), or 0 for a position that takes no part.  1 <= k <= min(kTopkMax, number of
// positions with a non-zero key).  On return (after a barrier) sh.items[0 .. k) hold the k best, best first; position of
// entry t = ~(unsigned)(sh.items[t] & 0xffffffff).
template <typename KeyAt>
__device__ __forceinline__ void topk_select_sort(KeyAt key_at, int n, int k, TopkShared& sh) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Q = ceil_div(ceil_div(n, 4), 64) * 64;
  const int p_begin = min(n, wave * Q), p_end = min(n, p_begin + Q);

  unsigned int prefix = 0u, pmask = 0u, rem = (unsigned int)k;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int i = tid; i < 4 * 256; i += 256) (&sh.hist[0][0])[i] = 0u;
    __syncthreads();
    for (int p0 = p_begin; p0 < p_end; p0 += 64) {
      const int p = p0 + lane;
      if (p < p_end) {
        const unsigned int key = key_at(p);
        if (key != 0u && (key & pmask) == prefix) atomicAdd(&sh.hist[wave][(key >> shift) & 255u], 1u);
      }
    }
    __syncthreads();
    if (wave == 0) {  // lane l owns the digits 255 - 4l .. 252 - 4l: counts above each digit by a 64-lane scan
      unsigned int c[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int d = 255 - (4 * lane + j);
        c[j] = sh.hist[0][d] + sh.hist[1][d] + sh.hist[2][d] + sh.hist[3][d];
      }
      const unsigned int mine = c[0] + c[1] + c[2] + c[3];
      unsigned int incl = mine;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
      }
      unsigned int above = incl - mine;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (above < rem && rem <= above + c[j]) {  // exactly one (lane, j): 1 <= rem <= the pass's total
          sh.sel[0] = 255u - (unsigned int)(4 * lane + j);
          sh.sel[1] = rem - above;
        }
        above += c[j];
      }
    }
    __syncthreads();
    const unsigned int d = sh.sel[0];
    rem = sh.sel[1];
    prefix |= d << shift;
    pmask |= 255u << shift;
    if (pass == 3 && tid < 4) sh.wave_eq[tid] = sh.hist[tid][d];
    if (pass == 3 && tid == 0) sh.n_above = 0u;
    __syncthreads();
  }
  // prefix = the k-th largest key; rem = how many keys equal to it belong to the result (the first by position)
  const unsigned int thr = prefix, ties = rem, above_total = (unsigned int)k - ties;
  unsigned int eq_seen = 0u;
  for (int w = 0; w < wave; ++w) eq_seen += sh.wave_eq[w];
  int n_sort = 1;
  while (n_sort < k) n_sort <<= 1;
  for (int i = k + tid; i < n_sort; i += 256) sh.items[i] = 0ull;  // padding: below every real key, after every position
  for (int p0 = p_begin; p0 < p_end; p0 += 64) {
    const int p = p0 + lane;
    const unsigned int key = p < p_end ? key_at(p) : 0u;
    const bool gt = p < p_end && key > thr, eq = p < p_end && key == thr;
    const unsigned long long m_gt = __ballot(gt), m_eq = __ballot(eq);
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned int base = 0u;
    if (lane == 0 && m_gt) base = atomicAdd(&sh.n_above, (unsigned int)__popcll(m_gt));
    base = __shfl(base, 0, 64);
    unsigned int slot = 0xffffffffu;
    if (gt) slot = base + (unsigned int)__popcll(m_gt & below);
    if (eq) {
      const unsigned int r = eq_seen + (unsigned int)__popcll(m_eq & below);
      if (r < ties) slot = above_total + r;
    }
    if (slot < (unsigned int)k) sh.items[slot] = ((unsigned long long)key << 32) | (unsigned int)~(unsigned int)p;
    eq_seen += (unsigned int)__popcll(m_eq);
  }
  for (int size = 2; size <= n_sort; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int i = tid; i < (n_sort >> 1); i += 256) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const unsigned long long x = sh.items[lo], y = sh.items[hi];
        const bool desc = (lo & size) == 0;
        if (desc ? x < y : x > y) { sh.items[lo] = y; sh.items[hi] = x; }
      }
    }
  }
  __syncthreads();
}
