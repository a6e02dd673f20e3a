// MIST pseudo-ground-truth mining (no grad): WSOVODROIHeads.get_pgt_mist (roi_heads.py:910-1040, sam=None) =
// get_pgt_top_k(top_k = 0.15, thres = 0.05) (:1043-1213) + class-agnostic NMS at 0.2, followed by
// label_and_sample_proposals_wsl (:1722-1825) with Matcher([thr], [0, 1]).
//
// Index and compare work, HBM / latency bound, no MFMA.  Three kernels around the existing wsovod_nms_segments:
//   mist_select_kernel  one workgroup per (image, image-level class): valid count, k, top-k of the class's score column
//                       over the valid rows (topk_select.h), score floor -> a descending (score, proposal) list
//   mist_merge_kernel   one workgroup per image: counting merge of the image's class lists into one descending candidate
//                       list (boxes, scores, classes, proposal index), capacity-padded, + the NMS segment offsets
//   [wsovod_nms_segments over one segment per image]
//   mist_label_kernel   grid over (256 proposals, image): the NMS survivors are the targets; every proposal is matched
//                       against all of them, tiled through LDS 128 at a time; block 0 of an image publishes its targets
// Nothing is read back by the host in between: counts live on the device, storage is sized by host-known capacities.
#include "common.h"
#include "topk_select.h"

// Index results must match the reference bit for bit: no mul+add fusion anywhere in this file.
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ int find_image(const int* __restrict__ off, int G, int t) {
  int lo = 0, hi = G;  // off[lo] <= t < off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- steps 1-5: per (image, class) candidate list ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void mist_select_kernel(const float* __restrict__ scores, long long ld,
                                                          const float4* __restrict__ boxes, const int* __restrict__ seg,
                                                          int G, const long long* __restrict__ gt_cls,
                                                          const int* __restrict__ gt_off, int K, double top_pro,
                                                          float thres, int k_cap, float* __restrict__ sel_scores,
                                                          int* __restrict__ sel_index, int* __restrict__ sel_len) {
  __shared__ TopkShared sh;
  __shared__ int s_red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = blockIdx.x;
  const int g = find_image(gt_off, G, t);
  const int m0 = seg[g], R = seg[g + 1] - m0;
  const long long cls = gt_cls[t];
  if (cls < 0 || cls >= K) {  // not a class of this head: no candidates (the host front refuses such lists where it can)
    if (tid == 0) sel_len[t] = 0;
    return;
  }
  const float* col = scores + (long long)m0 * ld + cls;
  const float4* bx = boxes + m0;
  auto valid = [&](int p) {  // roi_heads.py:1090-1096: area > 20, the same for every class
    const float4 b = bx[p];
    return (b.z - b.x) * (b.w - b.y) > 20.f;
  };
  int n = 0;
  for (int p = tid; p < R; p += 256) n += valid(p) ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if (lane == 0) s_red[wave] = n;
  __syncthreads();
  n = s_red[0] + s_red[1] + s_red[2] + s_red[3];
  if (n == 0) {
    if (tid == 0) sel_len[t] = 0;
    return;
  }
  // max(int(n * top_pro), 1) as Python computes it (roi_heads.py:1119): the product of IEEE doubles, truncated
  int k = max((int)((double)n * top_pro), 1);
  k = min(min(k, n), k_cap);
  topk_select_sort([&](int p) { return valid(p) ? topk_key(col[(long long)p * ld]) : 0u; }, R, k, sh);
  // score floor (:1148-1154): rank 0 always, rank r >= 1 iff score >= thres.  A NaN ranks first and fails the test, so
  // the kept ranks need not be a prefix: one wavefront compacts them in rank order
  if (wave == 0) {
    const long long out0 = (long long)t * k_cap;
    int kept = 0;
    for (int r0 = 0; r0 < k; r0 += 64) {
      const int r = r0 + lane;
      float s = 0.f;
      unsigned int p = 0u;
      bool keep = false;
      if (r < k) {
        p = ~(unsigned int)(sh.items[r] & 0xffffffffull);
        s = col[(long long)p * ld];  // the value itself: the key folds -0.0 and the NaN payloads
        keep = r == 0 || s >= thres;
      }
      const unsigned long long m = __ballot(keep);
      if (keep) {
        const int o = kept + __popcll(m & ((1ull << lane) - 1ull));
        sel_scores[out0 + o] = s;
        sel_index[out0 + o] = (int)p;
      }
      kept += __popcll(m);
    }
    if (lane == 0) sel_len[t] = kept;
  }
}

// ---- step 5-6 (input side): one descending candidate list per image ---------------------------------------------------
// Image g owns candidate rows [gt_off[g] * k_cap, gt_off[g + 1] * k_cap); list j of the image = slot gt_off[g] + j.  The
// lists' keys are staged in LDS; every element counts, list by list with two binary searches, the elements ahead of it:
// a higher score, or an equal one at a lower rank, or at the same rank in a lower class slot (the reference flattens the
// (rank, class) matrix row-major, :1175-1177, and the NMS visits equal scores in that order).  Places are a permutation
// of [0, count); rows from count up to the capacity are zeroed and marked invalid.
__global__ __launch_bounds__(1024) void mist_merge_kernel(const float* __restrict__ sel_scores,
                                                          const int* __restrict__ sel_index,
                                                          const int* __restrict__ sel_len, const float4* __restrict__ boxes,
                                                          const int* __restrict__ seg, const long long* __restrict__ gt_cls,
                                                          const int* __restrict__ gt_off, int G, int max_classes,
                                                          int k_cap, float4* __restrict__ cand_boxes,
                                                          float* __restrict__ cand_scores,
                                                          long long* __restrict__ cand_classes,
                                                          int* __restrict__ cand_index, unsigned char* __restrict__ cand_valid,
                                                          int* __restrict__ cand_count, int* __restrict__ nms_seg) {
  extern __shared__ unsigned int keys[];  // [C][k_cap]
  const int g = blockIdx.x, tid = threadIdx.x;
  const int c0 = gt_off[g], C = min(gt_off[g + 1] - c0, max_classes);  // (the LDS holds max_classes lists)
  const int m0 = seg[g];
  const long long row0 = (long long)c0 * k_cap;
  int total = 0;
  for (int j = 0; j < C; ++j) total += min(k_cap, max(0, sel_len[c0 + j]));
  for (int e = tid; e < C * k_cap; e += 1024) {
    const int j = e / k_cap, r = e - j * k_cap;
    if (r < min(k_cap, max(0, sel_len[c0 + j]))) keys[e] = topk_key(sel_scores[row0 + e]);
  }
  __syncthreads();
  for (int e = tid; e < C * k_cap; e += 1024) {
    const int j = e / k_cap, r = e - j * k_cap;
    if (r >= min(k_cap, max(0, sel_len[c0 + j]))) continue;
    const unsigned int s = keys[e];
    int place = r;
    for (int h = 0; h < C; ++h) {
      if (h == j) continue;
      const unsigned int* lst = keys + h * k_cap;
      const int len = min(k_cap, max(0, sel_len[c0 + h]));
      int lo = 0, hi = len;  // a = first rank whose key is not above s
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (lst[mid] > s) lo = mid + 1; else hi = mid;
      }
      const int a = lo;
      hi = len;              // b = first rank whose key is below s
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (lst[mid] >= s) lo = mid + 1; else hi = mid;
      }
      // of the equal run [a, b): ranks below r, and rank r itself in a lower slot
      place += a + max(0, min(lo, r + (h < j ? 1 : 0)) - a);
    }
    const int p = sel_index[row0 + e];
    const long long o = row0 + place;
    cand_boxes[o] = boxes[m0 + p];
    cand_scores[o] = sel_scores[row0 + e];
    cand_classes[o] = gt_cls[c0 + j];
    cand_index[o] = p;
    cand_valid[o] = 1;
  }
  for (int e = total + tid; e < C * k_cap; e += 1024) {
    const long long o = row0 + e;
    cand_boxes[o] = make_float4(0.f, 0.f, 0.f, 0.f);
    cand_scores[o] = 0.f;
    cand_classes[o] = 0;
    cand_index[o] = -1;
    cand_valid[o] = 0;
  }
  if (tid == 0) {
    cand_count[g] = total;
    nms_seg[g] = (int)row0;
    if (g == G - 1) nms_seg[G] = gt_off[G] * k_cap;
  }
}

// ---- steps 7-9: targets = NMS survivors; label every proposal against all of them ---------------------------------------
constexpr int kMistChunk = 128;  // targets staged in LDS at a time

__global__ __launch_bounds__(256) void mist_label_kernel(
    const float4* __restrict__ boxes, const int* __restrict__ seg, const int* __restrict__ gt_off, int k_cap,
    const float4* __restrict__ cand_boxes, const float* __restrict__ cand_scores, const long long* __restrict__ cand_classes,
    const int* __restrict__ cand_index, const int* __restrict__ cand_count, const int* __restrict__ keep_idx,
    const int* __restrict__ keep_count, int K, float iou_thr, float4* __restrict__ pgt_boxes,
    long long* __restrict__ pgt_classes, float* __restrict__ pgt_scores, float* __restrict__ pgt_weights,
    int* __restrict__ pgt_index, int* __restrict__ pgt_count, long long* __restrict__ out_classes,
    float4* __restrict__ out_boxes, float* __restrict__ out_scores, float* __restrict__ out_weights,
    int* __restrict__ out_matched) {
  __shared__ float4 s_box[kMistChunk];
  const int g = blockIdx.y, tid = threadIdx.x;
  const int m0 = seg[g], m1 = seg[g + 1];
  if ((long long)blockIdx.x * 256 >= (long long)(m1 - m0) && blockIdx.x != 0) return;  // (uniform: before any barrier)
  const int c0 = gt_off[g], cap = (gt_off[g + 1] - c0) * k_cap;
  const long long row0 = (long long)c0 * k_cap;
  // no valid box in the image (or no class): the dummy target of get_pgt_top_k's fallback (:1181-1207)
  const bool dummy = cand_count[g] <= 0;
  const int cnt = dummy ? 1 : min(max(keep_count[g], 0), cap);
  const float4 dbox = make_float4(-10000.f, -10000.f, 10000.f, 10000.f);
  const bool publish = blockIdx.x == 0;
  // an image without a class slot owns no target row: its proposals are still labelled against the dummy (staged in LDS),
  // but its published count is 0, so that nobody cuts the next image's rows for it
  if (publish && tid == 0) pgt_count[g] = min(cnt, cap);
  const int m = m0 + blockIdx.x * 256 + tid;
  const bool live = m < m1;
  float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) b = boxes[m];
  const float a1 = (b.z - b.x) * (b.w - b.y);
  float best = -1.f;
  int bj = 0;
  for (int j0 = 0; j0 < cnt; j0 += kMistChunk) {
    const int nj = min(kMistChunk, cnt - j0);
    __syncthreads();
    if (tid < nj) {
      const int j = j0 + tid;
      long long src = 0;
      float4 tb = dbox;
      if (!dummy) {
        src = row0 + min(max(keep_idx[row0 + j], 0), cap - 1);
        tb = cand_boxes[src];
      }
      s_box[tid] = tb;
      if (publish && j < cap) {  // (an image without a class slot has no row: its dummy lives only in LDS)
        pgt_boxes[row0 + j] = tb;
        pgt_classes[row0 + j] = dummy ? 0ll : cand_classes[src];
        const float sc = dummy ? 1.f : cand_scores[src];
        pgt_scores[row0 + j] = sc;
        pgt_weights[row0 + j] = sc;  // get_pgt_mist zips pgt_scores in as the weights (:1035-1037)
        pgt_index[row0 + j] = dummy ? -1 : cand_index[src];
      }
    }
    __syncthreads();
    for (int jj = 0; jj < nj; ++jj) {
      const float4 tb = s_box[jj];
      const float iw = fminf(b.z, tb.z) - fmaxf(b.x, tb.x);
      const float ih = fminf(b.w, tb.w) - fmaxf(b.y, tb.y);
      const float inter = fmaxf(iw, 0.f) * fmaxf(ih, 0.f);
      const float a2 = (tb.z - tb.x) * (tb.w - tb.y);
      // detectron2 pairwise_iou(gt, proposals): inter / (area_gt + area_prop - inter)
      const float iou = inter > 0.f ? inter / (a2 + a1 - inter) : 0.f;
      if (iou > best) {  // first maximum, across chunks too
        best = iou;
        bj = j0 + jj;
      }
    }
  }
  if (!live) return;
  float4 tb = dbox;
  long long tc = 0;
  float ts = 1.f;
  if (!dummy) {
    const long long src = row0 + min(max(keep_idx[row0 + bj], 0), cap - 1);
    tb = cand_boxes[src];
    tc = cand_classes[src];
    ts = cand_scores[src];
  }
  out_classes[m] = best >= iou_thr ? tc : (long long)K;
  out_boxes[m] = tb;
  out_scores[m] = ts;
  out_weights[m] = ts;
  out_matched[m] = bj;
}

}  // namespace

extern "C" {

int wsovod_mist_select(const float* scores, long long ld_scores, const float* boxes, const int* seg_offsets, int G,
                       const long long* gt_classes_img, const int* gt_offsets, int T, int K, double top_pro, float thres,
                       int k_cap, float* sel_scores, int* sel_index, int* sel_len, wsovod_stream_t stream) {
  WS_CHECK_ARG(G >= 0 && T >= 0 && K >= 1 && k_cap >= 1 && ld_scores >= K, "wsovod_mist_select: bad size");
  WS_CHECK_ARG(top_pro > 0.0 && top_pro < 1.0, "wsovod_mist_select: top_pro %g is not in (0, 1)", top_pro);
  if (k_cap > kTopkMax) {
    wsovod::set_error("wsovod_mist_select: k_cap %d is above the %d pairs one workgroup sorts", k_cap, kTopkMax);
    return WSOVOD_ERR_UNSUPPORTED;
  }
  if (G == 0 || T == 0) return WSOVOD_OK;
  WS_CHECK_ARG(scores && boxes && seg_offsets && gt_classes_img && gt_offsets && sel_scores && sel_index && sel_len,
               "wsovod_mist_select: null pointer");
  WS_CHECK_ARG(((uintptr_t)boxes & 15) == 0, "wsovod_mist_select: boxes must be 16-byte aligned");
  WS_CHECK_ARG((long long)T * k_cap < (1ll << 31), "wsovod_mist_select: too large");
  static int slot = wsovod::prof_slot("mist_select");
  hipStream_t s = (hipStream_t)stream;
  wsovod::ProfScope prof(slot, s, 0.0, (double)T * k_cap * 8.0);
  hipLaunchKernelGGL(mist_select_kernel, dim3(T), dim3(256), 0, s, scores, ld_scores, (const float4*)boxes, seg_offsets, G,
                     gt_classes_img, gt_offsets, K, top_pro, thres, k_cap, sel_scores, sel_index, sel_len);
  WS_CHECK_LAUNCH("wsovod_mist_select");
  return WSOVOD_OK;
}

int wsovod_mist_merge(const float* sel_scores, const int* sel_index, const int* sel_len, const float* boxes,
                      const int* seg_offsets, const long long* gt_classes_img, const int* gt_offsets, int G, int T,
                      int max_classes, int k_cap, float* cand_boxes, float* cand_scores, long long* cand_classes,
                      int* cand_index, unsigned char* cand_valid, int* cand_count, int* nms_seg_offsets,
                      wsovod_stream_t stream) {
  WS_CHECK_ARG(G >= 0 && T >= 0 && max_classes >= 0 && k_cap >= 1, "wsovod_mist_merge: bad size");
  if (G == 0) return WSOVOD_OK;
  WS_CHECK_ARG(seg_offsets && gt_offsets && cand_count && nms_seg_offsets, "wsovod_mist_merge: null pointer");
  WS_CHECK_ARG(T == 0 || (sel_scores && sel_index && sel_len && boxes && gt_classes_img && cand_boxes && cand_scores &&
                          cand_classes && cand_index && cand_valid), "wsovod_mist_merge: null pointer");
  WS_CHECK_ARG((((uintptr_t)boxes | (uintptr_t)cand_boxes) & 15) == 0,
               "wsovod_mist_merge: boxes/cand_boxes must be 16-byte aligned");
  WS_CHECK_ARG((long long)T * k_cap < (1ll << 31), "wsovod_mist_merge: too large");
  const size_t lds = (size_t)max(max_classes, 1) * k_cap * sizeof(unsigned int);
  if (lds > 64 * 1024) {
    wsovod::set_error("wsovod_mist_merge: %d lists of up to %d candidates need %zu B of LDS", max_classes, k_cap, lds);
    return WSOVOD_ERR_UNSUPPORTED;
  }
  static int slot = wsovod::prof_slot("mist_merge");
  hipStream_t s = (hipStream_t)stream;
  wsovod::ProfScope prof(slot, s, 0.0, (double)T * k_cap * 45.0);
  hipLaunchKernelGGL(mist_merge_kernel, dim3(G), dim3(1024), lds, s, sel_scores, sel_index, sel_len, (const float4*)boxes,
                     seg_offsets, gt_classes_img, gt_offsets, G, max(max_classes, 1), k_cap, (float4*)cand_boxes, cand_scores, cand_classes,
                     cand_index, cand_valid, cand_count, nms_seg_offsets);
  WS_CHECK_LAUNCH("wsovod_mist_merge");
  return WSOVOD_OK;
}

int wsovod_mist_label(const float* boxes, const int* seg_offsets, int G, int max_rows, const int* gt_offsets, int k_cap,
                      const float* cand_boxes, const float* cand_scores, const long long* cand_classes,
                      const int* cand_index, const int* cand_count, const int* keep_idx, const int* keep_count, int K,
                      float iou_threshold, float* pgt_boxes, long long* pgt_classes, float* pgt_scores,
                      float* pgt_weights, int* pgt_index, int* pgt_count, long long* out_classes, float* out_boxes,
                      float* out_scores, float* out_weights, int* out_matched, wsovod_stream_t stream) {
  WS_CHECK_ARG(G >= 0 && max_rows >= 0 && k_cap >= 1 && K >= 1, "wsovod_mist_label: bad size");
  if (G == 0) return WSOVOD_OK;
  WS_CHECK_ARG(seg_offsets && gt_offsets && cand_count && keep_count && pgt_count, "wsovod_mist_label: null pointer");
  WS_CHECK_ARG(boxes && cand_boxes && cand_scores && cand_classes && cand_index && keep_idx && pgt_boxes && pgt_classes &&
               pgt_scores && pgt_weights && pgt_index && out_classes && out_boxes && out_scores && out_weights &&
               out_matched, "wsovod_mist_label: null pointer");
  WS_CHECK_ARG((((uintptr_t)boxes | (uintptr_t)cand_boxes | (uintptr_t)pgt_boxes | (uintptr_t)out_boxes) & 15) == 0,
               "wsovod_mist_label: box arrays must be 16-byte aligned");
  static int slot = wsovod::prof_slot("mist_label");
  hipStream_t s = (hipStream_t)stream;
  wsovod::ProfScope prof(slot, s, 0.0, (double)G * max_rows * 48.0);
  hipLaunchKernelGGL(mist_label_kernel, dim3(max(1, ceil_div(max_rows, 256)), G), dim3(256), 0, s, (const float4*)boxes,
                     seg_offsets, gt_offsets, k_cap, (const float4*)cand_boxes, cand_scores, cand_classes, cand_index,
                     cand_count, keep_idx, keep_count, K, iou_threshold, (float4*)pgt_boxes, pgt_classes, pgt_scores,
                     pgt_weights, pgt_index, pgt_count, out_classes, (float4*)out_boxes, out_scores, out_weights,
                     out_matched);
  WS_CHECK_LAUNCH("wsovod_mist_label");
  return WSOVOD_OK;
}

}  // extern "C"
