// Proposal-side index work of the detection path: greedy non-maximum suppression over score-sorted boxes
// (the RPN's per-image NMS, proposal_utils.py:123, and the per-class NMS of the eval tail,
// fast_rcnn_open_vocabulary.py:176) and the anchor -> proposal decode of the RPN (rpn.py:495-515).
//
// Everything here is HBM / latency bound integer and compare work -- no MFMA.  Results are index sets and
// must be bit-identical to the reference's, so every float expression is written with explicit
// round-to-nearest intrinsics (no FMA contraction) in the reference's operation order.
//
// NMS is two launches over SEGMENTS (one image of the RPN batch, or one (image, class) pair of the eval tail):
//   1. nms_mask_kernel   -- thread (i, c): 64-bit word c of box i's suppression row = which of the 64 boxes
//                           [64c, 64c+64) of i's segment, ranked after i, overlap it by more than the
//                           threshold.  All lanes of a wavefront walk the same 64 candidate boxes, so the
//                           candidate loads are wave-uniform (one request, broadcast).
//   2. nms_scan_kernel   -- one wavefront per segment walks the rows in score order.  The 'removed' bitmap lives
//                           in registers (lane l owns words l, l+64, ...); rows are staged 64 at a time through
//                           LDS by a second wavefront while the current chunk is scanned; the
//                           word that decides the current chunk is mirrored in a wave-uniform scalar, so the
//                           sequential dependency per row is one scalar bit test.  Kept positions are written in
//                           order (they stay sorted by score) and the scan stops at max_keep.
#include "common.h"
#include "topk_select.h"

// Index results (bins, keep sets, labels) must match the reference bit for bit: no mul+add fusion anywhere in this
// file (HIP's __fmul_rn & co. are plain operators and would still be contracted under the default fp-contract=fast).
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ int find_segment(const int* __restrict__ seg, int G, int i) {
  int lo = 0, hi = G;  // seg[lo] <= i < seg[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seg[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void nms_mask_kernel(const float4* __restrict__ boxes, const int* __restrict__ seg,
                                                       int G, int N, int W, float thr,
                                                       unsigned long long* __restrict__ mask) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  if (i >= N) return;
  const int s = find_segment(seg, G, i);
  const int s0 = seg[s], s1 = seg[s + 1];
  const int il = i - s0;
  const int j0 = c * 64;
  unsigned long long bits = 0ull;
  if (j0 + 63 > il && s0 + j0 < s1) {
    const float4 a = boxes[i];
    const float area_a = __fmul_rn(__fsub_rn(a.z, a.x), __fsub_rn(a.w, a.y));
    const int jend = min(64, s1 - s0 - j0);
    for (int b = max(0, il + 1 - j0); b < jend; ++b) {
      const float4 q = boxes[s0 + j0 + b];
      const float area_b = __fmul_rn(__fsub_rn(q.z, q.x), __fsub_rn(q.w, q.y));
      const float w = fmaxf(0.f, __fsub_rn(fminf(a.z, q.z), fmaxf(a.x, q.x)));
      const float h = fmaxf(0.f, __fsub_rn(fminf(a.w, q.w), fmaxf(a.y, q.y)));
      const float inter = __fmul_rn(w, h);
      const float ovr = __fdiv_rn(inter, __fsub_rn(__fadd_rn(area_a, area_b), inter));
      if (ovr > thr) bits |= 1ull << b;
    }
  }
  mask[(long long)i * W + c] = bits;
}

constexpr int kScanRegs = 4;  // 'removed' words per lane -> segments of up to 64 * 64 * 4 = 16384 boxes

__global__ __launch_bounds__(128) void nms_scan_kernel(const unsigned long long* __restrict__ mask,
                                                       const int* __restrict__ seg,
                                                       const unsigned char* __restrict__ valid, int W, int max_keep,
                                                       int* __restrict__ keep_idx, int* __restrict__ keep_count) {
  // wavefront 0 scans, wavefront 1 stages the next 64-row chunk meanwhile; one barrier per chunk
  extern __shared__ unsigned long long rows[];  // 2 x [64 rows][W words]
  __shared__ int done;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s0 = seg[blockIdx.x], n = seg[blockIdx.x + 1] - s0;
  const int Wn = (n + 63) >> 6;  // words (= chunks) this segment really uses
  auto load_chunk = [&](int t) {
    unsigned long long* dst = rows + (size_t)(t & 1) * 64 * W;
    const long long base = (long long)(s0 + t * 64) * W;
    const int live = min(64, n - t * 64) * W;
    for (int e = lane; e < live; e += 64) dst[e] = mask[base + e];
  };
  if (threadIdx.x == 0) done = 0;
  if (wave == 1 && Wn > 0) load_chunk(0);
  __syncthreads();
  unsigned long long remv[kScanRegs] = {0ull, 0ull, 0ull, 0ull};
  int count = 0;
  for (int t = 0; t < Wn; ++t) {
    if (wave == 1) {
      if (t + 1 < Wn) load_chunk(t + 1);
    } else {
      const unsigned long long* cur_rows = rows + (size_t)(t & 1) * 64 * W;
      const int rows_here = min(64, n - t * 64);
      // the word of the removed bitmap that covers this chunk, as a wave-uniform value
      unsigned long long mine = remv[0];
#pragma unroll
      for (int r = 1; r < kScanRegs; ++r)
        if ((t >> 6) == r) mine = remv[r];
      unsigned long long cur = __shfl(mine, t & 63, 64);
      if (valid) cur |= ~__ballot(lane < rows_here && valid[s0 + t * 64 + lane] != 0);
      for (int b = 0; b < rows_here; ++b) {
        if ((cur >> b) & 1ull) continue;
        if (lane == 0) keep_idx[s0 + count] = t * 64 + b;
        if (++count >= max_keep) break;
        const unsigned long long* row = cur_rows + (size_t)b * W;
        cur |= row[t];
#pragma unroll
        for (int r = 0; r < kScanRegs; ++r) {
          const int w = lane + 64 * r;
          if (w < Wn) remv[r] |= row[w];
        }
      }
      if (count >= max_keep && lane == 0) done = 1;
    }
    __syncthreads();
    if (done) break;
  }
  if (threadIdx.x == 0) keep_count[blockIdx.x] = count;
}

// Anchor -> proposal decode (Box2BoxTransform.apply_deltas, detectron2 box_regression.py; called
// from rpn.py:495-515) + clip to the image + the min-size test of find_top_rpn_proposals
// (proposal_utils.py:112-121).  One thread per selected anchor.  valid = finite && both sides > min_size.
__global__ __launch_bounds__(256) void rpn_decode_kernel(const float4* __restrict__ anchors,
                                                         const float4* __restrict__ deltas,
                                                         const long long* __restrict__ index, int per_image,
                                                         long long anchors_per_image, const float* __restrict__ sizes,
                                                         float wx, float wy, float ww, float wh, float scale_clamp,
                                                         float min_size, int total, float4* __restrict__ out,
                                                         unsigned char* __restrict__ valid) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int img = t / per_image;
  const long long a = index ? index[t] : (long long)(t - img * per_image);
  const float4 an = anchors[a];
  const float4 d = deltas[(long long)img * anchors_per_image + a];
  const float widths = __fsub_rn(an.z, an.x), heights = __fsub_rn(an.w, an.y);
  const float ctr_x = __fadd_rn(an.x, __fmul_rn(0.5f, widths)), ctr_y = __fadd_rn(an.y, __fmul_rn(0.5f, heights));
  const float dx = __fdiv_rn(d.x, wx), dy = __fdiv_rn(d.y, wy);
  const float dw = fminf(__fdiv_rn(d.z, ww), scale_clamp), dh = fminf(__fdiv_rn(d.w, wh), scale_clamp);
  const float pcx = __fadd_rn(__fmul_rn(dx, widths), ctr_x), pcy = __fadd_rn(__fmul_rn(dy, heights), ctr_y);
  const float pw = __fmul_rn(expf(dw), widths), ph = __fmul_rn(expf(dh), heights);
  float x1 = __fsub_rn(pcx, __fmul_rn(0.5f, pw)), y1 = __fsub_rn(pcy, __fmul_rn(0.5f, ph));
  float x2 = __fadd_rn(pcx, __fmul_rn(0.5f, pw)), y2 = __fadd_rn(pcy, __fmul_rn(0.5f, ph));
  const bool finite = isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2);
  const float H = sizes[2 * img], Wd = sizes[2 * img + 1];
  x1 = fminf(fmaxf(x1, 0.f), Wd); x2 = fminf(fmaxf(x2, 0.f), Wd);
  y1 = fminf(fmaxf(y1, 0.f), H);  y2 = fminf(fmaxf(y2, 0.f), H);
  out[t] = make_float4(x1, y1, x2, y2);
  valid[t] = finite && __fsub_rn(x2, x1) > min_size && __fsub_rn(y2, y1) > min_size;
}

// Patch rows of the RPN's 3x3 conv for the weight gradient: only the <= BATCH_SIZE_PER_IMAGE sampled anchors of
// an image carry a loss, so dW = dH_act^T . im2col(x)[act] needs the im2col rows of those pixels only
// (rpn.py:296-375 -> label == -1 anchors contribute nothing).  One workgroup per selected output pixel, 16-byte
// chunks; taps outside the map and rows with index < 0 are zero.
template <typename T>
__global__ __launch_bounds__(256) void im2col_rows_kernel(const T* __restrict__ x, const long long* __restrict__ rows,
                                                          int H, int W, int Cin, int Ho, int Wo, int KH, int KW,
                                                          int stride, int pad, int dil, T* __restrict__ out) {
  constexpr int EPC = 16 / (int)sizeof(T);
  const long long r = rows[blockIdx.x];
  const int cpc = Cin / EPC;               // chunks per tap
  const int chunks = KH * KW * cpc;
  uint4* dst = (uint4*)(out + (long long)blockIdx.x * KH * KW * Cin);
  int img = 0, ho = 0, wo = 0;
  if (r >= 0) {
    img = (int)(r / ((long long)Ho * Wo));
    const int rem = (int)(r - (long long)img * Ho * Wo);
    ho = rem / Wo;
    wo = rem - ho * Wo;
  }
  for (int c = threadIdx.x; c < chunks; c += 256) {
    const int tap = c / cpc, cc = c - tap * cpc;
    const int kh = tap / KW, kw = tap - kh * KW;
    const int hi = ho * stride - pad + kh * dil, wi = wo * stride - pad + kw * dil;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (r >= 0 && hi >= 0 && hi < H && wi >= 0 && wi < W)
      v = *(const uint4*)(x + (((long long)img * H + hi) * W + wi) * Cin + cc * EPC);
    dst[c] = v;
  }
}

// Anchor labelling of the RPN (rpn.py:237-293 with detectron2's Matcher(allow_low_quality_matches=True) and
// pairwise_iou restated).  Pass 1: every (image, anchor) takes the best-overlapping pseudo-GT
// box of its image and raises that box's best-IoU cell (IoUs are >= 0, so their bit patterns order like unsigned
// ints).  Pass 2: thresholds -> {0, -1, 1}, then the low-quality rule: an anchor that attains some box's best IoU
// is positive whatever its own maximum.  Both passes evaluate the same fp32 expression, so the equality is exact.
// noinline: both passes must execute the very same instruction sequence for the equality test to be exact.
__device__ __attribute__((noinline)) float box_iou_d2(const float4 g, const float area_g, const float4 a,
                                                      const float area_a) {
  const float w = fmaxf(__fsub_rn(fminf(g.z, a.z), fmaxf(g.x, a.x)), 0.f);
  const float h = fmaxf(__fsub_rn(fminf(g.w, a.w), fmaxf(g.y, a.y)), 0.f);
  const float inter = __fmul_rn(w, h);
  return inter > 0.f ? __fdiv_rn(inter, __fsub_rn(__fadd_rn(area_g, area_a), inter)) : 0.f;
}

__global__ __launch_bounds__(256) void rpn_match_kernel(const float4* __restrict__ anchors, int A,
                                                        const float4* __restrict__ gt, const int* __restrict__ gt_start,
                                                        const int* __restrict__ gt_count,
                                                        float* __restrict__ best_val, int* __restrict__ best_gt,
                                                        unsigned int* __restrict__ gt_best) {
  const int a = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (a >= A) return;
  const float4 an = anchors[a];
  const float area_a = __fmul_rn(__fsub_rn(an.z, an.x), __fsub_rn(an.w, an.y));
  const int g0 = gt_start[b], g1 = g0 + gt_count[b];
  float best = -1.f;
  int arg = -1;
  for (int g = g0; g < g1; ++g) {
    const float4 q = gt[g];
    const float iou = box_iou_d2(q, __fmul_rn(__fsub_rn(q.z, q.x), __fsub_rn(q.w, q.y)), an, area_a);
    if (iou > best) { best = iou; arg = g; }
    atomicMax(gt_best + g, __float_as_uint(iou));
  }
  best_val[(long long)b * A + a] = best;
  best_gt[(long long)b * A + a] = arg;
}

__global__ __launch_bounds__(256) void rpn_label_kernel(const float4* __restrict__ anchors, int A,
                                                        const float4* __restrict__ gt, const int* __restrict__ gt_start,
                                                        const int* __restrict__ gt_count,
                                                        const float* __restrict__ best_val,
                                                        const unsigned int* __restrict__ gt_best, float lo, float hi,
                                                        signed char* __restrict__ labels) {
  const int a = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (a >= A) return;
  const int g0 = gt_start[b], g1 = g0 + gt_count[b];
  const float v = best_val[(long long)b * A + a];
  signed char lab = 0;  // no box at all: background (Matcher's empty-matrix default)
  if (g1 > g0) {
    lab = v >= hi ? 1 : (v >= lo ? -1 : 0);
    const float4 an = anchors[a];
    const float area_a = __fmul_rn(__fsub_rn(an.z, an.x), __fsub_rn(an.w, an.y));
    for (int g = g0; g < g1; ++g) {
      const float4 q = gt[g];
      const float iou = box_iou_d2(q, __fmul_rn(__fsub_rn(q.z, q.x), __fsub_rn(q.w, q.y)), an, area_a);
      if (__float_as_uint(iou) == gt_best[g]) lab = 1;
    }
  }
  labels[(long long)b * A + a] = lab;
}

// ---- grouped top-k of the MRRP RPN (proposal_utils.py:199-239: per level and per anchor id, sort the H*W logits of
// that anchor and keep min(H*W, pre_nms_topk)) ------------------------------------------------------------------------
// One workgroup per (row b, anchor a); the row is the HW values logits[b][p][a], stride A.  Order and equality are
// torch.sort's (descending, stable); selection and sort are topk_select.h's, then coalesced stores of score and flat
// index p * A + a.
__global__ __launch_bounds__(256) void rpn_group_topk_kernel(const float* __restrict__ logits, int HW, int A, int k,
                                                             float* __restrict__ out_scores,
                                                             long long* __restrict__ out_index) {
  __shared__ TopkShared sh;
  const int tid = threadIdx.x;
  const int b = blockIdx.x / A, a = blockIdx.x - b * A;
  const float* row = logits + ((long long)b * HW) * A + a;
  topk_select_sort([&](int p) { return topk_key(row[(long long)p * A]); }, HW, k, sh);
  const long long out0 = (long long)blockIdx.x * k;
  for (int t = tid; t < k; t += 256) {
    const unsigned int p = ~(unsigned int)(sh.items[t] & 0xffffffffull);
    out_scores[out0 + t] = row[(long long)p * A];  // the value itself: the key folds -0.0 and the NaN payloads
    out_index[out0 + t] = (long long)p * A + a;
  }
}

// ---- k-way merge of the per-(level, anchor) NMS survivors (proposal_utils.py:335-351: batched_nms returns the kept boxes
// of all groups sorted by score, of which the first post_nms_topk are kept) -------------------------------------------
// One workgroup per image.  List g of the image = the keep_count[n*G+g] positions keep_idx[(n*G+g)*k ...] that
// wsovod_nms_segments wrote, already by descending score.  The kept scores are staged in LDS; every kept element then
// counts, list by list with a binary search, the elements ahead of it (equal scores: lower group first), which is its
// place in the output.  Places are a permutation, so every output row below `count` is written exactly once.
__global__ __launch_bounds__(1024) void nms_merge_groups_kernel(const float4* __restrict__ boxes,
                                                                const float* __restrict__ scores,
                                                                const int* __restrict__ keep_idx,
                                                                const int* __restrict__ keep_count, int G, int A, int k,
                                                                int cap, int post, float4* __restrict__ out_boxes,
                                                                float* __restrict__ out_scores,
                                                                long long* __restrict__ out_ids,
                                                                int* __restrict__ out_count) {
  extern __shared__ float kept[];  // [G][cap], cap = min(post, k): the longest list
  const int n = blockIdx.x, tid = threadIdx.x;
  const long long seg0 = (long long)n * G;
  int total = 0;
  for (int g = 0; g < G; ++g) total += min(cap, max(0, keep_count[seg0 + g]));
  for (int e = tid; e < G * cap; e += 1024) {
    const int g = e / cap, r = e - g * cap;
    const int len = min(cap, max(0, keep_count[seg0 + g]));
    if (r < len) {
      const int rel = keep_idx[(seg0 + g) * k + r];
      kept[e] = scores[(seg0 + g) * k + min(max(rel, 0), k - 1)];
    }
  }
  __syncthreads();
  for (int e = tid; e < G * cap; e += 1024) {
    const int g = e / cap, r = e - g * cap;
    const int len = min(cap, max(0, keep_count[seg0 + g]));
    if (r >= len) continue;
    const float s = kept[e];
    int place = r;
    for (int h = 0; h < G && place < post; ++h) {
      if (h == g) continue;
      const float* lst = kept + h * cap;
      int lo = 0, hi = min(cap, max(0, keep_count[seg0 + h]));
      // first position whose element does NOT go ahead of (g, r): ahead = score > s, or == s in a lower group
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const float v = lst[mid];
        if (v > s || (v == s && h < g)) lo = mid + 1; else hi = mid;
      }
      place += lo;
    }
    if (place < post) {
      const int rel = min(max(keep_idx[(seg0 + g) * k + r], 0), k - 1);
      const long long o = (long long)n * post + place;
      out_boxes[o] = boxes[(seg0 + g) * k + rel];
      out_scores[o] = s;
      out_ids[o] = (long long)(g / A) * 1000 + (g % A);
    }
  }
  if (tid == 0) out_count[n] = min(post, total);
}

}  // namespace

extern "C" {

int wsovod_rpn_group_topk(const float* logits, int B, int HW, int A, int pre_nms_topk, float* scores, long long* index,
                          wsovod_stream_t stream) {
  WS_CHECK_ARG(B >= 0 && HW >= 0 && A >= 0 && pre_nms_topk >= 1, "wsovod_rpn_group_topk: bad size");
  if (pre_nms_topk > kTopkMax) {
    wsovod::set_error("wsovod_rpn_group_topk: pre_nms_topk %d is above the %d pairs one workgroup sorts", pre_nms_topk,
                      kTopkMax);
    return WSOVOD_ERR_UNSUPPORTED;
  }
  if (B == 0 || HW == 0 || A == 0) return WSOVOD_OK;
  WS_CHECK_ARG(logits && scores && index, "wsovod_rpn_group_topk: null pointer");
  WS_CHECK_ARG((long long)B * A < (1ll << 31) && (long long)HW + 256 < (1ll << 31), "wsovod_rpn_group_topk: too large");
  const int k = min(HW, pre_nms_topk);
  static int slot = wsovod::prof_slot("rpn_group_topk");
  hipStream_t s = (hipStream_t)stream;
  wsovod::ProfScope prof(slot, s, 0.0, 6.0 * B * HW * A * 4 + 12.0 * B * A * k);
  hipLaunchKernelGGL(rpn_group_topk_kernel, dim3(B * A), dim3(256), 0, s, logits, HW, A, k, scores, index);
  WS_CHECK_LAUNCH("wsovod_rpn_group_topk");
  return WSOVOD_OK;
}

int wsovod_nms_merge_groups(const float* boxes, const float* scores, const int* keep_idx, const int* keep_count,
                            int num_images, int G, int A, int seg_len, int post_nms_topk, float* out_boxes,
                            float* out_scores, long long* out_level_ids, int* out_count, wsovod_stream_t stream) {
  WS_CHECK_ARG(num_images >= 0 && G >= 1 && A >= 1 && G % A == 0 && seg_len >= 0 && post_nms_topk >= 1,
               "wsovod_nms_merge_groups: bad size");
  if (num_images == 0) return WSOVOD_OK;
  WS_CHECK_ARG(keep_count && out_count, "wsovod_nms_merge_groups: null pointer");
  WS_CHECK_ARG(seg_len == 0 || (boxes && scores && keep_idx && out_boxes && out_scores && out_level_ids),
               "wsovod_nms_merge_groups: null pointer");
  WS_CHECK_ARG((((uintptr_t)boxes | (uintptr_t)out_boxes) & 15) == 0,
               "wsovod_nms_merge_groups: boxes/out_boxes must be 16-byte aligned");
  const int post = post_nms_topk, cap = max(1, min(post_nms_topk, seg_len));  // a list holds at most seg_len elements
  const size_t lds = (size_t)G * cap * sizeof(float);
  if (lds > 150 * 1024 || (long long)num_images * G * max(seg_len, 1) >= (1ll << 31)) {
    wsovod::set_error("wsovod_nms_merge_groups: %d lists of up to %d kept scores need %zu B of LDS", G, cap, lds);
    return WSOVOD_ERR_UNSUPPORTED;
  }
  if (lds > 64 * 1024)  // the opt-in is per device and cheap: asked for on every launch that needs it, no process-wide flag
    WS_CHECK_HIP(hipFuncSetAttribute((const void*)nms_merge_groups_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     150 * 1024), "wsovod_nms_merge_groups: LDS opt-in");
  static int slot = wsovod::prof_slot("nms_merge_groups");
  hipStream_t s = (hipStream_t)stream;
  wsovod::ProfScope prof(slot, s, 0.0, (double)num_images * G * cap * 28.0);
  hipLaunchKernelGGL(nms_merge_groups_kernel, dim3(num_images), dim3(1024), lds, s, (const float4*)boxes, scores,
                     keep_idx, keep_count, G, A, max(seg_len, 1), cap, post, (float4*)out_boxes, out_scores, out_level_ids,
                     out_count);
  WS_CHECK_LAUNCH("wsovod_nms_merge_groups");
  return WSOVOD_OK;
}

int wsovod_rpn_label_anchors(const float* anchors, int A, const float* gt_boxes, const int* gt_start,
                             const int* gt_count, int num_images, int total_gt, float thr_lo, float thr_hi, float* best_iou, int* best_gt,
                             unsigned int* gt_best_ws, signed char* labels, wsovod_stream_t stream) {
  if (num_images == 0 || A == 0) return WSOVOD_OK;
  WS_CHECK_ARG(anchors && gt_start && gt_count && best_iou && best_gt && labels,
               "wsovod_rpn_label_anchors: null pointer");
  WS_CHECK_ARG(total_gt == 0 || (gt_boxes && gt_best_ws), "wsovod_rpn_label_anchors: null pointer");
  WS_CHECK_ARG((((uintptr_t)anchors | (uintptr_t)gt_boxes) & 15) == 0,
               "wsovod_rpn_label_anchors: anchors/gt_boxes must be 16-byte aligned");
  static int slot = wsovod::prof_slot("rpn_label_anchors");
  hipStream_t s = (hipStream_t)stream;
  wsovod::ProfScope prof(slot, s, 0.0, (double)num_images * A * 25.0);
  if (total_gt > 0 && hipMemsetAsync(gt_best_ws, 0, sizeof(unsigned int) * total_gt, s) != hipSuccess) {
    wsovod::set_error("wsovod_rpn_label_anchors: memset failed");
    return WSOVOD_ERR_HIP;
  }
  const dim3 grid(ceil_div(A, 256), num_images);
  hipLaunchKernelGGL(rpn_match_kernel, grid, dim3(256), 0, s, (const float4*)anchors, A, (const float4*)gt_boxes,
                     gt_start, gt_count, best_iou, best_gt, gt_best_ws);
  hipLaunchKernelGGL(rpn_label_kernel, grid, dim3(256), 0, s, (const float4*)anchors, A, (const float4*)gt_boxes,
                     gt_start, gt_count, best_iou, gt_best_ws, thr_lo, thr_hi, labels);
  WS_CHECK_LAUNCH("wsovod_rpn_label_anchors");
  return WSOVOD_OK;
}

int wsovod_im2col_rows(const void* x, int dtype, const long long* rows, int n_rows, int H, int W, int Cin, int Ho, int Wo,
                       int KH, int KW, int stride, int pad, int dil, void* out, wsovod_stream_t stream) {
  if (n_rows == 0) return WSOVOD_OK;
  WS_CHECK_ARG(x && rows && out, "wsovod_im2col_rows: null pointer");
  const int esz = dtype == WSOVOD_BF16 ? 2 : 4;
  WS_CHECK_ARG(dtype == WSOVOD_BF16 || dtype == WSOVOD_F32, "wsovod_im2col_rows: bad dtype");
  WS_CHECK_ARG(Cin % (16 / esz) == 0, "wsovod_im2col_rows: Cin=%d must be a multiple of %d", Cin, 16 / esz);
  WS_CHECK_ARG((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "wsovod_im2col_rows: x/out must be 16-byte aligned");
  static int slot = wsovod::prof_slot("im2col_rows");
  hipStream_t s = (hipStream_t)stream;
  wsovod::ProfScope prof(slot, s, 0.0, 2.0 * n_rows * KH * KW * Cin * esz);
  if (dtype == WSOVOD_BF16)
    hipLaunchKernelGGL(im2col_rows_kernel<bf16_t>, dim3(n_rows), dim3(256), 0, s, (const bf16_t*)x, rows, H, W, Cin, Ho,
                       Wo, KH, KW, stride, pad, dil, (bf16_t*)out);
  else
    hipLaunchKernelGGL(im2col_rows_kernel<float>, dim3(n_rows), dim3(256), 0, s, (const float*)x, rows, H, W, Cin, Ho,
                       Wo, KH, KW, stride, pad, dil, (float*)out);
  WS_CHECK_LAUNCH("wsovod_im2col_rows");
  return WSOVOD_OK;
}

int wsovod_nms_segments(const float* boxes, const int* seg_offsets, const unsigned char* valid, int G, int N,
                        int max_seg_len, float iou_threshold, int max_keep, unsigned long long* workspace,
                        int* keep_idx, int* keep_count, wsovod_stream_t stream) {
  WS_CHECK_ARG(G >= 0 && N >= 0 && max_seg_len >= 0, "wsovod_nms_segments: negative size");
  if (G == 0) return WSOVOD_OK;
  WS_CHECK_ARG(seg_offsets && keep_idx && keep_count, "wsovod_nms_segments: null pointer");
  WS_CHECK_ARG(N == 0 || (boxes && workspace), "wsovod_nms_segments: null pointer");
  WS_CHECK_ARG(((uintptr_t)boxes & 15) == 0, "wsovod_nms_segments: boxes must be 16-byte aligned");
  const int W = max(1, ceil_div(max_seg_len, 64));
  if (W > 64 * kScanRegs) {
    wsovod::set_error("wsovod_nms_segments: segments of more than %d boxes are not supported (got %d)",
                      64 * 64 * kScanRegs, max_seg_len);
    return WSOVOD_ERR_UNSUPPORTED;
  }
  const size_t lds = (size_t)2 * 64 * W * sizeof(unsigned long long);
  if (lds > 159 * 1024) {
    wsovod::set_error("wsovod_nms_segments: max_seg_len %d needs %zu B of LDS", max_seg_len, lds);
    return WSOVOD_ERR_UNSUPPORTED;
  }
  if (max_keep <= 0) max_keep = 0x7fffffff;
  hipStream_t s = (hipStream_t)stream;
  static int slot_m = wsovod::prof_slot("nms_mask"), slot_s = wsovod::prof_slot("nms_scan");
  if (N > 0) {
    wsovod::ProfScope prof(slot_m, s, 0.0, (double)N * W * 8 + (double)N * 16);
    hipLaunchKernelGGL(nms_mask_kernel, dim3(ceil_div(N, 256), W), dim3(256), 0, s, (const float4*)boxes, seg_offsets,
                       G, N, W, iou_threshold, workspace);
    WS_CHECK_LAUNCH("wsovod_nms_segments(mask)");
  }
  {
    static bool attr_set = false;
    if (!attr_set) {
      WS_OPT_IN_LDS(nms_scan_kernel, 159 * 1024, "wsovod_nms_segments: LDS opt-in");
      attr_set = true;
    }
    wsovod::ProfScope prof(slot_s, s, 0.0, (double)N * W * 8);
    hipLaunchKernelGGL(nms_scan_kernel, dim3(G), dim3(128), lds, s, workspace, seg_offsets, valid, W, max_keep,
                       keep_idx, keep_count);
    WS_CHECK_LAUNCH("wsovod_nms_segments(scan)");
  }
  return WSOVOD_OK;
}

int wsovod_rpn_decode(const float* anchors, const float* deltas, const long long* index, int num_images, int per_image,
                      long long anchors_per_image, const float* image_sizes, const float* weights, float scale_clamp,
                      float min_size, float* boxes, unsigned char* valid, wsovod_stream_t stream) {
  const long long total = (long long)num_images * per_image;
  if (total == 0) return WSOVOD_OK;
  WS_CHECK_ARG(total < (1ll << 31), "wsovod_rpn_decode: too many boxes");
  WS_CHECK_ARG(anchors && deltas && image_sizes && weights && boxes && valid, "wsovod_rpn_decode: null pointer");
  WS_CHECK_ARG((((uintptr_t)anchors | (uintptr_t)deltas | (uintptr_t)boxes) & 15) == 0,
               "wsovod_rpn_decode: anchors/deltas/boxes must be 16-byte aligned");
  static int slot = wsovod::prof_slot("rpn_decode");
  hipStream_t s = (hipStream_t)stream;
  wsovod::ProfScope prof(slot, s, 0.0, (double)total * 57);
  hipLaunchKernelGGL(rpn_decode_kernel, dim3(ceil_div((int)total, 256)), dim3(256), 0, s, (const float4*)anchors,
                     (const float4*)deltas, index, per_image, anchors_per_image, image_sizes, weights[0], weights[1],
                     weights[2], weights[3], scale_clamp, min_size, (int)total, (float4*)boxes, valid);
  WS_CHECK_LAUNCH("wsovod_rpn_decode");
  return WSOVOD_OK;
}

}  // extern "C"
