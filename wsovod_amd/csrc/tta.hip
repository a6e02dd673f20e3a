// Test-time augmentation on the device (MODEL.HIP.TTA_DEVICE): the view builder and the merge around the per-view forwards.
//
//   wsovod_resample_u8    PIL.Image.resize(..., BILINEAR) of a uint8 (3, H, W) image, bit for bit: Pillow's 8-bit path is a
//                         separable 22-bit fixed-point filter whose horizontal pass rounds and clamps to uint8 before the
//                         vertical pass reads it, so the two passes are two kernels with a uint8 intermediate.  The
//                         coefficient tables come from the host (fp64, wsovod_amd/layers/hip_ops.py:resample_table).
//   wsovod_tta_map_boxes  TransformList.inverse().apply_box of a view's boxes in float32, operation by operation.
//   wsovod_tta_avg        that mapping for up to 32 views of the same proposals plus the mean over the views (fp64 sum in
//                         view order, one division, one rounding to float32) of boxes and class scores, one launch.
//
// Every float32 product / difference of the mapping is an explicit round-to-nearest intrinsic: hipcc would contract
// `W - x * s` into an FMA, and the result has to equal numpy's separate operations.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;  // Pillow's PRECISION_BITS

__device__ __forceinline__ unsigned char clip8(int acc) {
  int v = acc >> kPrecisionBits;  // arithmetic shift: a negative sum stays negative and clamps to 0
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// One output sample of a pass: taps bounds[2 * o] .. + bounds[2 * o + 1] of a line with `stride` bytes between taps.
// A table that points outside the line (never built by the host side) reads nothing instead of reading out of bounds.
__device__ __forceinline__ unsigned char filter_tap(const unsigned char* line, long long stride, int in_size, const int* kk,
                                                    const int* bounds, int ksize, int o) {
  int first = bounds[2 * o], n = bounds[2 * o + 1];
  if (first < 0 || n < 0 || n > ksize || first + n > in_size) n = 0;
  const int* k = kk + (long long)o * ksize;
  const unsigned char* p = line + first * stride;
  int acc = 1 << (kPrecisionBits - 1);
  for (int t = 0; t < n; ++t) acc += (int)p[t * stride] * k[t];
  return clip8(acc);
}

// Horizontal pass: src (rows, W) -> dst (rows, nw), rows = 3 * H.  A thread owns four consecutive bytes of the flat output
// (one 4-byte store; the four may lie on two rows), the tail thread stores its 1..3 bytes one by one.
__global__ void __launch_bounds__(256) resample_h_kernel(const unsigned char* __restrict__ src, int W, int nw,
                                                         const int* __restrict__ kk, const int* __restrict__ bounds, int ksize,
                                                         long long total, unsigned char* __restrict__ dst) {
  const long long i0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i0 >= total) return;
  unsigned char v[4];
  const int cnt = (int)(total - i0 < 4 ? total - i0 : 4);
  long long row = i0 / nw;
  int x = (int)(i0 - row * nw);
  for (int j = 0; j < cnt; ++j) {
    v[j] = filter_tap(src + row * W, 1, W, kk, bounds, ksize, x);
    if (++x == nw) { x = 0; ++row; }
  }
  if (cnt == 4) {
    *reinterpret_cast<uchar4*>(dst + i0) = make_uchar4(v[0], v[1], v[2], v[3]);
  } else {
    for (int j = 0; j < cnt; ++j) dst[i0 + j] = v[j];
  }
}

// Vertical pass: src (3, H, nw) -> out slice 0 (3, nh, nw) and, with `mirror`, slice 1 = slice 0 with every row reversed,
// in the same launch.  kk == nullptr: the axis keeps its size and the pass is a copy (nh == H).
__global__ void __launch_bounds__(256) resample_v_kernel(const unsigned char* __restrict__ src, int H, int nh, int nw,
                                                         const int* __restrict__ kk, const int* __restrict__ bounds, int ksize,
                                                         long long total, int mirror, unsigned char* __restrict__ out) {
  const long long i0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i0 >= total) return;
  unsigned char v[4];
  const int cnt = (int)(total - i0 < 4 ? total - i0 : 4);
  long long row = i0 / nw;  // c * nh + y
  int x = (int)(i0 - row * nw);
  unsigned char* flipped = out + total;
  for (int j = 0; j < cnt; ++j) {
    const int c = (int)(row / nh), y = (int)(row - (long long)c * nh);
    const unsigned char* col = src + (long long)c * H * nw + x;
    v[j] = kk ? filter_tap(col, nw, H, kk, bounds, ksize, y) : col[(long long)y * nw];
    if (mirror) flipped[row * nw + (nw - 1 - x)] = v[j];
    if (++x == nw) { x = 0; ++row; }
  }
  if (cnt == 4) {
    *reinterpret_cast<uchar4*>(out + i0) = make_uchar4(v[0], v[1], v[2], v[3]);
  } else {
    for (int j = 0; j < cnt; ++j) out[i0 + j] = v[j];
  }
}

// np.min / np.max over the corner list: a NaN wins, as numpy's reductions propagate it.
__device__ __forceinline__ float np_min(float a, float b) { return (a != a) ? a : ((b != b) ? b : (b < a ? b : a)); }
__device__ __forceinline__ float np_max(float a, float b) { return (a != a) ? a : ((b != b) ? b : (b > a ? b : a)); }

__device__ __forceinline__ float map_x(float x, const wsovod_tta_xform& t) {
  if (t.flip) x = __fsub_rn(t.flip_w, x);
  x = __fmul_rn(x, t.sx);
  if (t.has_pre) x = __fmul_rn(x, t.px);
  return x;
}
__device__ __forceinline__ float map_y(float y, const wsovod_tta_xform& t) {
  y = __fmul_rn(y, t.sy);
  if (t.has_pre) y = __fmul_rn(y, t.py);
  return y;
}
__device__ __forceinline__ float4 map_box(float4 b, const wsovod_tta_xform& t) {
  const float x0 = map_x(b.x, t), x1 = map_x(b.z, t), y0 = map_y(b.y, t), y1 = map_y(b.w, t);
  return make_float4(np_min(x0, x1), np_min(y0, y1), np_max(x0, x1), np_max(y0, y1));
}

__global__ void __launch_bounds__(256) tta_map_boxes_kernel(const float4* __restrict__ boxes, int M, wsovod_tta_xform t,
                                                            float4* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < M) out[i] = map_box(boxes[i], t);
}

// Threads [0, n_box) average one box each, threads [n_box, n_box + n_score) one score each.
__global__ void __launch_bounds__(256) tta_avg_kernel(wsovod_tta_views views, int n_box, int n_score,
                                                      float4* __restrict__ mean_boxes, float* __restrict__ mean_scores) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int V = views.n_views;
  if (i < n_box) {
    double ax = 0.0, ay = 0.0, az = 0.0, aw = 0.0;
    for (int v = 0; v < V; ++v) {
      const float4 b = map_box(reinterpret_cast<const float4*>(views.v[v].boxes)[i], views.v[v].xf);
      ax += (double)b.x;
      ay += (double)b.y;
      az += (double)b.z;
      aw += (double)b.w;
    }
    const double d = (double)V;
    mean_boxes[i] = make_float4((float)(ax / d), (float)(ay / d), (float)(az / d), (float)(aw / d));
  } else if (i - n_box < n_score) {
    const int j = i - n_box;
    double a = 0.0;
    for (int v = 0; v < V; ++v) a += (double)views.v[v].scores[j];
    mean_scores[j] = (float)(a / (double)V);
  }
}

}  // namespace

extern "C" {

int wsovod_resample_u8(const unsigned char* src, int H, int W, int nh, int nw, const int* kk_h, const int* bounds_h,
                       int ksize_h, const int* kk_v, const int* bounds_v, int ksize_v, unsigned char* tmp,
                       unsigned char* out, int flip, wsovod_stream_t stream) {
  WS_CHECK_ARG(H > 0 && W > 0 && nh > 0 && nw > 0, "wsovod_resample_u8: sizes must be positive (%d x %d -> %d x %d)", H, W,
               nh, nw);
  WS_CHECK_ARG(src && out, "wsovod_resample_u8: null pointer");
  const bool pass_h = nw != W, pass_v = nh != H;
  WS_CHECK_ARG(pass_h == (kk_h != nullptr) && pass_h == (bounds_h != nullptr) && (!pass_h || (ksize_h > 0 && tmp)),
               "wsovod_resample_u8: a horizontal table and the workspace are needed exactly when the width changes");
  WS_CHECK_ARG(pass_v == (kk_v != nullptr) && pass_v == (bounds_v != nullptr) && (!pass_v || ksize_v > 0),
               "wsovod_resample_u8: a vertical table is needed exactly when the height changes");
  WS_CHECK_ARG((((uintptr_t)out | (uintptr_t)tmp) & 3) == 0, "wsovod_resample_u8: tmp / out must be 4-byte aligned");
  const long long n_mid = 3ll * H * nw, n_out = 3ll * nh * nw, n_src = 3ll * H * W;
  const long long cap = 1ll << 31;  // 4 bytes a thread, 256 threads a block: the grid stays far below 2^31 blocks
  if (n_mid >= cap || n_out >= cap || n_src >= cap || (long long)nw * ksize_h >= cap || (long long)nh * ksize_v >= cap) {
    wsovod::set_error("wsovod_resample_u8: %d x %d -> %d x %d is beyond 2^31 bytes per tensor or table", H, W, nh, nw);
    return WSOVOD_ERR_UNSUPPORTED;
  }
  hipStream_t s = (hipStream_t)stream;
  const unsigned char* mid = src;
  if (pass_h) {
    static int slot_h = wsovod::prof_slot("tta_resample_h");
    wsovod::ProfScope prof(slot_h, s, 0.0, (double)n_src + (double)n_mid);
    hipLaunchKernelGGL(resample_h_kernel, dim3((unsigned)ceil_div_ll(n_mid, 1024)), dim3(256), 0, s, src, W, nw, kk_h,
                       bounds_h, ksize_h, n_mid, tmp);
    WS_CHECK_LAUNCH("wsovod_resample_u8(horizontal)");
    mid = tmp;
  }
  static int slot_v = wsovod::prof_slot("tta_resample_v");
  wsovod::ProfScope prof(slot_v, s, 0.0, (double)n_mid + (double)n_out * (flip ? 2 : 1));
  hipLaunchKernelGGL(resample_v_kernel, dim3((unsigned)ceil_div_ll(n_out, 1024)), dim3(256), 0, s, mid, H, nh, nw, kk_v,
                     bounds_v, ksize_v, n_out, flip ? 1 : 0, out);
  WS_CHECK_LAUNCH("wsovod_resample_u8(vertical)");
  return WSOVOD_OK;
}

int wsovod_tta_map_boxes(const float* boxes, int M, const wsovod_tta_xform* xform, float* out, wsovod_stream_t stream) {
  WS_CHECK_ARG(M >= 0 && xform, "wsovod_tta_map_boxes: M >= 0 and a transform are needed");
  if (M == 0) return WSOVOD_OK;
  WS_CHECK_ARG(boxes && out, "wsovod_tta_map_boxes: null pointer");
  WS_CHECK_ARG((((uintptr_t)boxes | (uintptr_t)out) & 15) == 0, "wsovod_tta_map_boxes: boxes / out must be 16-byte aligned");
  static int slot = wsovod::prof_slot("tta_map_boxes");
  hipStream_t s = (hipStream_t)stream;
  wsovod::ProfScope prof(slot, s, 0.0, (double)M * 32);
  hipLaunchKernelGGL(tta_map_boxes_kernel, dim3(ceil_div(M, 256)), dim3(256), 0, s, (const float4*)boxes, M, *xform,
                     (float4*)out);
  WS_CHECK_LAUNCH("wsovod_tta_map_boxes");
  return WSOVOD_OK;
}

int wsovod_tta_avg(const wsovod_tta_views* views, int R, int box_cols, int score_cols, float* mean_boxes,
                   float* mean_scores, wsovod_stream_t stream) {
  WS_CHECK_ARG(views, "wsovod_tta_avg: null view table");
  if (views->n_views > WSOVOD_TTA_MAX_VIEWS) {
    wsovod::set_error("wsovod_tta_avg: %d views, the by-value table holds %d", views->n_views, WSOVOD_TTA_MAX_VIEWS);
    return WSOVOD_ERR_UNSUPPORTED;
  }
  WS_CHECK_ARG(views->n_views >= 1, "wsovod_tta_avg: at least one view");
  WS_CHECK_ARG(R >= 0 && box_cols >= 0 && box_cols % 4 == 0 && score_cols >= 0,
               "wsovod_tta_avg: R >= 0, box_cols a multiple of 4, score_cols >= 0");
  const long long n_box = (long long)R * (box_cols / 4), n_score = (long long)R * score_cols;
  if (n_box + n_score == 0) return WSOVOD_OK;
  WS_CHECK_ARG(n_box + n_score < (1ll << 31), "wsovod_tta_avg: too many elements");
  WS_CHECK_ARG((n_box == 0 || mean_boxes) && (n_score == 0 || mean_scores), "wsovod_tta_avg: null output");
  WS_CHECK_ARG(((uintptr_t)mean_boxes & 15) == 0, "wsovod_tta_avg: mean_boxes must be 16-byte aligned");
  for (int v = 0; v < views->n_views; ++v) {
    WS_CHECK_ARG((n_box == 0 || views->v[v].boxes) && (n_score == 0 || views->v[v].scores),
                 "wsovod_tta_avg: view %d has a null pointer", v);
    WS_CHECK_ARG(((uintptr_t)views->v[v].boxes & 15) == 0, "wsovod_tta_avg: view %d: boxes must be 16-byte aligned", v);
  }
  static int slot = wsovod::prof_slot("tta_avg");
  hipStream_t s = (hipStream_t)stream;
  wsovod::ProfScope prof(slot, s, 0.0, (double)(n_box * 16 + n_score * 4) * (views->n_views + 1));
  hipLaunchKernelGGL(tta_avg_kernel, dim3((unsigned)ceil_div_ll(n_box + n_score, 256)), dim3(256), 0, s, *views, (int)n_box,
                     (int)n_score, (float4*)mean_boxes, mean_scores);
  WS_CHECK_LAUNCH("wsovod_tta_avg");
  return WSOVOD_OK;
}

}  // extern "C"
