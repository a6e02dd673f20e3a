// Training input stage on the device (MODEL.HIP.INPUT_DEVICE): what the reference's DatasetMapper does per image on the host
// (data/dataset_mapper.py:144-191 -- ResizeShortestEdge, RandomFlip, transform_proposals -- and the zero padding of
// ImageList.from_tensors), for a whole batch in a fixed number of launches.
//
//   wsovod_resample_u8_batch    wsovod_resample_u8 (tta.hip: Pillow's 8-bit bilinear resize, byte for byte) for up to 32 images
//                               in two launches, blockIdx.y = image: one horizontal pass into per-image uint8 intermediates,
//                               one vertical pass that writes each image's canvas slot completely (image, mirrored on request,
//                               and the zero padding around it).  A byte-granular, memory-bound gather: a thread owns one
//                               aligned 4-byte word of its output; the canvas slots and rows are not 4-byte aligned in general
//                               (odd Wp), so the words are aligned to the allocation and a slot's partial first / last word is
//                               stored byte by byte -- the neighbouring slot's threads own the other bytes of that word.
//   wsovod_transform_proposals  detection_utils.transform_proposals (:222-265) per image segment: apply_box, clip, unique_boxes
//                               (first occurrence = minimum row per hash key, atomicMin on an open-addressed table in global
//                               memory), nonempty, top-k, dense write.  One workgroup scans a segment 256 rows at a time, so a
//                               segment's length is not bounded by LDS.
//
// The random crop (MODEL.HIP.INPUT_CROP; dataset_mapper.py:88-89, T.RandomCrop in front of the list) adds no kernel: the
// resample kernels read every source through a window (byte strides, a start and a size -- wsovod_resample_u8_batch_win; the
// entry without a window passes the whole image), the proposal kernel subtracts the crop offset first
// (wsovod_transform_proposals_win; the entry without one passes has_crop = 0).
//
// Every float32 product / difference is an explicit round-to-nearest intrinsic (see tta.hip): numpy's separate operations.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;  // Pillow's PRECISION_BITS

__device__ __forceinline__ unsigned char clip8(int acc) {
  int v = acc >> kPrecisionBits;  // arithmetic shift: a negative sum stays negative and clamps to 0
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// One output sample of a pass (tta.hip:filter_tap): a table row that points outside the line reads nothing.
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

// Byte strides (channel, row, pixel) of an image's source: the window's own.  Plane-major or interleaved, whole image or crop:
// the kernels know strides only.
struct Strides {
  long long c, y, x;
};
__device__ __forceinline__ Strides src_strides(const wsovod_resample_window& d) { return {d.stride_c, d.stride_y, d.stride_x}; }

// Horizontal pass of image blockIdx.y: src -> its plane-major (3, H, nw) intermediate.  Four consecutive bytes a thread, one
// 4-byte store (tmp offsets are multiples of 4); blocks past the image's end, or of an image that keeps its width, leave.
__global__ void __launch_bounds__(256) resample_batch_h_kernel(wsovod_resample_window_batch b, const int* __restrict__ tables,
                                                               unsigned char* __restrict__ scratch) {
  const wsovod_resample_window& d = b.img[blockIdx.y];
  if (d.ksize_h == 0) return;
  const long long total = 3ll * d.H * d.nw;
  const long long i0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i0 >= total) return;
  const Strides st = src_strides(d);
  const int* kk = tables + d.kk_h;
  const int* bounds = tables + d.bounds_h;
  unsigned char* dst = scratch + d.tmp;
  unsigned char v[4];
  const int cnt = (int)(total - i0 < 4 ? total - i0 : 4);
  long long row = i0 / d.nw;  // c * H + y
  int x = (int)(i0 - row * d.nw);
  for (int j = 0; j < cnt; ++j) {
    const int c = (int)(row / d.H), y = (int)(row - (long long)c * d.H);
    v[j] = filter_tap(d.src + c * st.c + y * st.y, st.x, d.W, kk, bounds, d.ksize_h, x);
    if (++x == d.nw) { x = 0; ++row; }
  }
  if (cnt == 4) {
    *reinterpret_cast<uchar4*>(dst + i0) = make_uchar4(v[0], v[1], v[2], v[3]);
  } else {
    for (int j = 0; j < cnt; ++j) dst[i0 + j] = v[j];
  }
}

// Vertical pass of image blockIdx.y: its intermediate (or its source, when the width is kept) -> slot blockIdx.y of the canvas,
// every byte of the slot: the image in [0, nh) x [0, nw) -- output column x reads column nw - 1 - x with the flip bit -- and
// zero elsewhere.  Thread t owns the aligned word at (slot base rounded down to 4) + 4 t, clipped to the slot.
__global__ void __launch_bounds__(256) resample_batch_v_kernel(wsovod_resample_window_batch b, const int* __restrict__ tables,
                                                               const unsigned char* __restrict__ scratch,
                                                               unsigned char* __restrict__ canvas, int Hp, int Wp) {
  const wsovod_resample_window& d = b.img[blockIdx.y];
  const long long slot = 3ll * Hp * Wp;
  unsigned char* base = canvas + (long long)blockIdx.y * slot;
  const int lead = (int)((uintptr_t)base & 3);
  const long long w0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4 - lead;  // slot-relative, < 0 for a partial first word
  if (w0 >= slot) return;
  const unsigned char* mid;
  Strides st;
  if (d.ksize_h) {
    mid = scratch + d.tmp;
    st = {(long long)d.H * d.nw, d.nw, 1};
  } else {
    mid = d.src;
    st = src_strides(d);  // (W == nw)
  }
  const int* kk = tables + d.kk_v;
  const int* bounds = tables + d.bounds_v;
  const bool flip = d.flip != 0;
  const long long i_first = w0 < 0 ? 0 : w0;
  const long long i_end = w0 + 4 < slot ? w0 + 4 : slot;
  long long row = i_first / Wp;  // c * Hp + y
  int x = (int)(i_first - row * Wp);
  unsigned char v[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long i = w0 + j;
    if (i < i_first || i >= i_end) continue;
    const int c = (int)(row / Hp), y = (int)(row - (long long)c * Hp);
    if (y < d.nh && x < d.nw) {
      const unsigned char* col = mid + c * st.c + (flip ? d.nw - 1 - x : x) * st.x;
      v[j] = d.ksize_v ? filter_tap(col, st.y, d.H, kk, bounds, d.ksize_v, y) : col[y * st.y];
    }
    if (++x == Wp) { x = 0; ++row; }
  }
  if (i_first == w0 && i_end == w0 + 4) {
    *reinterpret_cast<uchar4*>(base + w0) = make_uchar4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (w0 + j >= i_first && w0 + j < i_end) base[w0 + j] = v[j];
    }
  }
}

// ---- proposals ----

constexpr long long kEmptyKey = -1;  // (0xFF bytes: the table is cleared with one memset; a real key is >= 0)

struct ProposalWs {
  long long* keys;     // (T) hash keys, kEmptyKey = free
  unsigned int* rows;  // (T) minimum segment-relative row of the key
  float4* mapped;      // (total_rows) transformed and clipped boxes
  int* slot;           // (total_rows) table entry of the row's key
  unsigned int mask;   // T - 1, T a power of two >= 2 * total_rows
};

static inline long long table_entries(long long total_rows) {
  long long t = 64;
  while (t < 2 * total_rows) t <<= 1;
  return t;
}

__device__ __forceinline__ float clampf(float v, float hi) { return v < 0.0f ? 0.0f : (v > hi ? hi : v); }

__device__ __forceinline__ unsigned int mix64(unsigned long long k) {  // (splitmix64's finaliser)
  k ^= k >> 30;
  k *= 0xbf58476d1ce4e5b9ull;
  k ^= k >> 27;
  k *= 0x94d049bb133111ebull;
  k ^= k >> 31;
  return (unsigned int)k;
}

// Steps 1-3a of a row: apply_box, clip, hash key, and the key's table entry with the minimum row that carries it.
__global__ void __launch_bounds__(256) proposals_map_kernel(wsovod_proposal_window_batch b, const float4* __restrict__ boxes,
                                                            ProposalWs ws) {
  const int g = blockIdx.y;
  const wsovod_proposal_window& d = b.img[g];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.count) return;
  const int r = d.start + i;
  float4 bx = boxes[r];
  if (d.has_crop) {  // CropTransform.apply_coords: float32 differences of their own, in front of the scale
    bx.x = __fsub_rn(bx.x, d.crop_x);
    bx.z = __fsub_rn(bx.z, d.crop_x);
    bx.y = __fsub_rn(bx.y, d.crop_y);
    bx.w = __fsub_rn(bx.w, d.crop_y);
  }
  float xa = __fmul_rn(bx.x, d.sx), xb = __fmul_rn(bx.z, d.sx);
  const float ya = __fmul_rn(bx.y, d.sy), yb = __fmul_rn(bx.w, d.sy);
  if (d.flip) {
    xa = __fsub_rn(d.flip_w, xa);
    xb = __fsub_rn(d.flip_w, xb);
  }
  float4 m;
  m.x = clampf(xb < xa ? xb : xa, d.clip_w);
  m.y = clampf(yb < ya ? yb : ya, d.clip_h);
  m.z = clampf(xb > xa ? xb : xa, d.clip_w);
  m.w = clampf(yb > ya ? yb : ya, d.clip_h);
  ws.mapped[r] = m;
  // np.round is round-half-even, as rintf under the default rounding mode; the image index keeps the segments' keys apart
  const long long key = (long long)rintf(m.x) + 1000ll * (long long)rintf(m.y) + 1000000ll * (long long)rintf(m.z) +
                        1000000000ll * (long long)rintf(m.w) + ((long long)g << 53);
  unsigned int h = mix64((unsigned long long)key) & ws.mask;
  for (unsigned int probe = 0; probe <= ws.mask; ++probe) {  // (load factor <= 1/2: a free entry is always met)
    const long long prev = (long long)atomicCAS(reinterpret_cast<unsigned long long*>(ws.keys + h),
                                                (unsigned long long)kEmptyKey, (unsigned long long)key);
    if (prev == kEmptyKey || prev == key) {
      atomicMin(ws.rows + h, (unsigned int)i);
      ws.slot[r] = (int)h;
      return;
    }
    h = (h + 1) & ws.mask;
  }
  ws.slot[r] = -1;  // (never reached; the select kernel drops such a row instead of reading outside the table)
}

// Steps 3b-5 of image blockIdx.x: 256 rows at a time, keep = first of its key and non-empty, block-wide exclusive scan of the
// keep flags on top of the running count, scatter of the ranks below topk; then the count and the zeroed tail of the slot.
__global__ void __launch_bounds__(256) proposals_select_kernel(wsovod_proposal_window_batch b, const float* __restrict__ logits,
                                                               ProposalWs ws, int topk, float4* __restrict__ out_boxes,
                                                               float* __restrict__ out_logits, int* __restrict__ out_count) {
  __shared__ int wave_total[4];
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const wsovod_proposal_window& d = b.img[g];
  float4* ob = out_boxes + (long long)g * topk;
  float* ol = out_logits + (long long)g * topk;
  int run = 0;
  for (int c0 = 0; c0 < d.count && run < topk; c0 += 256) {
    const int i = c0 + tid;
    bool keep = false;
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
    int r = 0;
    if (i < d.count) {
      r = d.start + i;
      m = ws.mapped[r];
      const unsigned int e = (unsigned int)ws.slot[r];
      keep = e <= ws.mask && ws.rows[e] == (unsigned int)i && __fsub_rn(m.z, m.x) > 0.0f && __fsub_rn(m.w, m.y) > 0.0f;
    }
    const unsigned long long votes = __ballot(keep);
    const int before = __popcll(votes & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[wave] = __popcll(votes);
    __syncthreads();
    int offset = run, total = 0;
    for (int w = 0; w < 4; ++w) {
      if (w < wave) offset += wave_total[w];
      total += wave_total[w];
    }
    const int rank = offset + before;
    if (keep && rank < topk) {
      ob[rank] = m;
      ol[rank] = logits[r];
    }
    run += total;  // (the same value in every thread: the loop condition is uniform)
    __syncthreads();
  }
  const int count = run < topk ? run : topk;
  for (int j = count + tid; j < topk; j += 256) {
    ob[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    ol[j] = 0.f;
  }
  if (tid == 0) out_count[g] = count;
}

bool whole_in_range(float v, float lo) { return v >= lo && v <= 4.0e6f && v == (float)(long long)v; }

// Both resample entries behind their own null / image-count checks: validation of every image against the tables, the
// scratch, the canvas and the window's readable bytes, then the two launches.  `who` names the entry in messages.
int resample_windows(const char* who, const wsovod_resample_window_batch& b, const int* tables, long long table_ints,
                     unsigned char* scratch, long long scratch_bytes, unsigned char* canvas, int Hp, int Wp,
                     wsovod_stream_t stream) {
  WS_CHECK_ARG(b.n >= 1 && Hp > 0 && Wp > 0 && canvas, "%s: at least one image and a canvas", who);
  WS_CHECK_ARG(table_ints >= 0 && scratch_bytes >= 0, "%s: negative table / scratch size", who);
  WS_CHECK_ARG((((uintptr_t)canvas | (uintptr_t)scratch) & 3) == 0, "%s: scratch / canvas must be 4-byte aligned", who);
  const long long cap = 1ll << 31;
  const long long slot = 3ll * Hp * Wp;
  if (slot >= cap) {
    wsovod::set_error("%s: a %d x %d canvas slot is beyond 2^31 bytes", who, Hp, Wp);
    return WSOVOD_ERR_UNSUPPORTED;
  }
  long long max_mid = 0;
  for (int g = 0; g < b.n; ++g) {
    const wsovod_resample_window& d = b.img[g];
    WS_CHECK_ARG(d.src && d.H > 0 && d.W > 0 && d.nh > 0 && d.nw > 0,
                 "%s: image %d: a source and positive sizes are needed (%d x %d -> %d x %d)", who, g, d.H, d.W, d.nh, d.nw);
    WS_CHECK_ARG(d.nh <= Hp && d.nw <= Wp, "%s: image %d: %d x %d does not fit the %d x %d canvas", who, g, d.nh, d.nw, Hp, Wp);
    WS_CHECK_ARG((d.ksize_h > 0) == (d.nw != d.W) && d.ksize_h >= 0 && (d.ksize_v > 0) == (d.nh != d.H) && d.ksize_v >= 0,
                 "%s: image %d: an axis has a table (ksize > 0) exactly when its size changes", who, g);
    const long long n_src = 3ll * d.H * d.W, n_mid = 3ll * d.H * d.nw;
    if (n_src >= cap || n_mid >= cap || (long long)d.nw * d.ksize_h >= cap || (long long)d.nh * d.ksize_v >= cap) {
      wsovod::set_error("%s: image %d: %d x %d -> %d x %d is beyond 2^31 bytes per tensor or table", who, g, d.H, d.W, d.nh,
                        d.nw);
      return WSOVOD_ERR_UNSUPPORTED;
    }
    WS_CHECK_ARG(d.stride_c > 0 && d.stride_y > 0 && (d.stride_x == 1 || d.stride_x == 3),
                 "%s: image %d: byte strides (%lld, %lld, %d): positive, the pixel stride 1 or 3", who, g, d.stride_c, d.stride_y,
                 d.stride_x);
    if (d.stride_c >= cap || d.stride_y >= cap) {
      wsovod::set_error("%s: image %d: a byte stride (%lld, %lld) of 2^31 or more", who, g, d.stride_c, d.stride_y);
      return WSOVOD_ERR_UNSUPPORTED;
    }
    // the window's last sample (channel 2, row H - 1, column W - 1); every term is below 2^62
    const long long last = 2 * d.stride_c + (d.H - 1) * d.stride_y + (d.W - 1) * (long long)d.stride_x;
    WS_CHECK_ARG(last < d.src_bytes, "%s: image %d: the window's last sample lies at byte %lld of the %lld readable ones", who, g,
                 last, d.src_bytes);
    if (d.ksize_h) {
      WS_CHECK_ARG(tables && d.kk_h >= 0 && d.kk_h + (long long)d.nw * d.ksize_h <= table_ints && d.bounds_h >= 0 &&
                       d.bounds_h + 2ll * d.nw <= table_ints,
                   "%s: image %d: the horizontal table lies outside the %lld table entries", who, g, table_ints);
      WS_CHECK_ARG(scratch && d.tmp >= 0 && d.tmp % 4 == 0 && d.tmp + n_mid <= scratch_bytes,
                   "%s: image %d: the intermediate (offset %lld, %lld bytes) lies outside the %lld scratch bytes or is not 4-byte "
                   "aligned", who, g, d.tmp, n_mid, scratch_bytes);
      for (int o = 0; o < g; ++o) {
        const wsovod_resample_window& e = b.img[o];
        WS_CHECK_ARG(!e.ksize_h || e.tmp + 3ll * e.H * e.nw <= d.tmp || d.tmp + n_mid <= e.tmp,
                     "%s: the intermediates of images %d and %d overlap", who, o, g);
      }
      if (n_mid > max_mid) max_mid = n_mid;
    }
    if (d.ksize_v) {
      WS_CHECK_ARG(tables && d.kk_v >= 0 && d.kk_v + (long long)d.nh * d.ksize_v <= table_ints && d.bounds_v >= 0 &&
                       d.bounds_v + 2ll * d.nh <= table_ints,
                   "%s: image %d: the vertical table lies outside the %lld table entries", who, g, table_ints);
    }
  }
  hipStream_t s = (hipStream_t)stream;
  if (max_mid > 0) {
    static int slot_h = wsovod::prof_slot("input_resample_h");
    double bytes = 0.0;
    for (int g = 0; g < b.n; ++g) {
      const wsovod_resample_window& d = b.img[g];
      if (d.ksize_h) bytes += 3.0 * d.H * d.W + 3.0 * d.H * d.nw;
    }
    wsovod::ProfScope prof(slot_h, s, 0.0, bytes);
    hipLaunchKernelGGL(resample_batch_h_kernel, dim3((unsigned)ceil_div_ll(max_mid, 1024), (unsigned)b.n), dim3(256), 0, s, b,
                       tables, scratch);
    WS_CHECK_LAUNCH(who);
  }
  static int slot_v = wsovod::prof_slot("input_resample_v");
  double bytes = (double)slot * b.n;
  for (int g = 0; g < b.n; ++g) bytes += 3.0 * b.img[g].H * b.img[g].nw;
  wsovod::ProfScope prof(slot_v, s, 0.0, bytes);
  hipLaunchKernelGGL(resample_batch_v_kernel, dim3((unsigned)ceil_div_ll(slot + 3, 1024), (unsigned)b.n), dim3(256), 0, s, b,
                     tables, scratch, canvas, Hp, Wp);
  WS_CHECK_LAUNCH(who);
  return WSOVOD_OK;
}

// Both proposal entries behind their own null / image-count checks.
int proposal_windows(const char* who, const wsovod_proposal_window_batch& b, const float* boxes, const float* logits,
                     int total_rows, int topk, void* workspace, long long workspace_bytes, float* out_boxes, float* out_logits,
                     int* out_count, wsovod_stream_t stream) {
  WS_CHECK_ARG(b.n >= 1 && topk >= 1 && total_rows >= 0 && total_rows < (1 << 30),
               "%s: at least one image, topk >= 1, 0 <= total_rows < 2^30", who);
  WS_CHECK_ARG(out_boxes && out_logits && out_count && workspace && (total_rows == 0 || (boxes && logits)), "%s: null pointer",
               who);
  WS_CHECK_ARG((((uintptr_t)boxes | (uintptr_t)out_boxes | (uintptr_t)workspace) & 15) == 0,
               "%s: boxes / out_boxes / workspace must be 16-byte aligned", who);
  WS_CHECK_ARG(workspace_bytes >= wsovod_transform_proposals_workspace_bytes(total_rows),
               "%s: the workspace has %lld bytes, %lld are needed", who, workspace_bytes,
               wsovod_transform_proposals_workspace_bytes(total_rows));
  WS_CHECK_ARG((long long)b.n * topk < (1ll << 28), "%s: n * topk too large", who);
  int max_count = 0;
  for (int g = 0; g < b.n; ++g) {
    const wsovod_proposal_window& d = b.img[g];
    WS_CHECK_ARG(d.start >= 0 && d.count >= 0 && (long long)d.start + d.count <= total_rows,
                 "%s: image %d: rows [%d, %d + %d) lie outside the %d rows", who, g, d.start, d.start, d.count, total_rows);
    if (!whole_in_range(d.clip_w, 1.0f) || !whole_in_range(d.clip_h, 1.0f)) {
      wsovod::set_error("%s: image %d: a %g x %g frame: whole sizes in [1, 4e6] only (the box hash is exact in int64 up to "
                        "there)", who, g, (double)d.clip_h, (double)d.clip_w);
      return WSOVOD_ERR_UNSUPPORTED;
    }
    if (d.has_crop && (!whole_in_range(d.crop_x, 0.0f) || !whole_in_range(d.crop_y, 0.0f))) {
      wsovod::set_error("%s: image %d: a crop offset of (%g, %g): whole numbers in [0, 4e6] only (the host subtracts an int)", who,
                        g, (double)d.crop_x, (double)d.crop_y);
      return WSOVOD_ERR_UNSUPPORTED;
    }
    if (d.count > max_count) max_count = d.count;
  }
  const long long n = total_rows, t = table_entries(n);
  ProposalWs ws;
  char* p = (char*)workspace;
  ws.keys = (long long*)p;
  ws.rows = (unsigned int*)(p + t * 8);
  ws.mapped = (float4*)(p + ((t * 12 + 15) / 16) * 16);
  ws.slot = (int*)((char*)ws.mapped + n * 16);
  ws.mask = (unsigned int)(t - 1);
  hipStream_t s = (hipStream_t)stream;
  if (max_count > 0) {
    WS_CHECK_HIP(hipMemsetAsync(workspace, 0xFF, (size_t)(t * 12), s), who);
    static int slot_m = wsovod::prof_slot("input_proposals_map");
    wsovod::ProfScope prof(slot_m, s, 0.0, (double)n * (16 + 16 + 4 + 24));
    hipLaunchKernelGGL(proposals_map_kernel, dim3(ceil_div(max_count, 256), b.n), dim3(256), 0, s, b, (const float4*)boxes, ws);
    WS_CHECK_LAUNCH(who);
  }
  static int slot_s = wsovod::prof_slot("input_proposals_select");
  wsovod::ProfScope prof(slot_s, s, 0.0, (double)n * 28 + (double)b.n * topk * 20);
  hipLaunchKernelGGL(proposals_select_kernel, dim3(b.n), dim3(256), 0, s, b, logits, ws, topk, (float4*)out_boxes, out_logits,
                     out_count);
  WS_CHECK_LAUNCH(who);
  return WSOVOD_OK;
}

}  // namespace

extern "C" {

int wsovod_resample_u8_batch(const wsovod_resample_batch* batch, const int* tables, long long table_ints,
                             unsigned char* scratch, long long scratch_bytes, unsigned char* canvas, int Hp, int Wp,
                             wsovod_stream_t stream) {
  static const char who[] = "wsovod_resample_u8_batch";
  WS_CHECK_ARG(batch, "%s: null image table", who);
  if (batch->n > WSOVOD_INPUT_MAX_IMAGES) {
    wsovod::set_error("%s: %d images, the by-value table holds %d", who, batch->n, WSOVOD_INPUT_MAX_IMAGES);
    return WSOVOD_ERR_UNSUPPORTED;
  }
  wsovod_resample_window_batch b = {};  // the whole image as its own window: the strides of its layout, all of its bytes readable
  b.n = batch->n;
  for (int g = 0; g < batch->n; ++g) {
    const wsovod_resample_image& d = batch->img[g];
    wsovod_resample_window& w = b.img[g];
    const bool inter = d.flags & WSOVOD_RESAMPLE_INTERLEAVED;
    w.src = d.src;
    w.src_bytes = 3ll * d.H * d.W;
    w.stride_c = inter ? 1 : (long long)d.H * d.W;
    w.stride_y = inter ? 3ll * d.W : d.W;
    w.stride_x = inter ? 3 : 1;
    w.H = d.H, w.W = d.W, w.nh = d.nh, w.nw = d.nw;
    w.flip = (d.flags & WSOVOD_RESAMPLE_FLIP) ? 1 : 0;
    w.kk_h = d.kk_h, w.bounds_h = d.bounds_h, w.ksize_h = d.ksize_h;
    w.kk_v = d.kk_v, w.bounds_v = d.bounds_v, w.ksize_v = d.ksize_v;
    w.tmp = d.tmp;
  }
  return resample_windows(who, b, tables, table_ints, scratch, scratch_bytes, canvas, Hp, Wp, stream);
}

int wsovod_resample_u8_batch_win(const wsovod_resample_window_batch* batch, const int* tables, long long table_ints,
                                 unsigned char* scratch, long long scratch_bytes, unsigned char* canvas, int Hp, int Wp,
                                 wsovod_stream_t stream) {
  static const char who[] = "wsovod_resample_u8_batch_win";
  WS_CHECK_ARG(batch, "%s: null image table", who);
  if (batch->n > WSOVOD_INPUT_MAX_IMAGES) {
    wsovod::set_error("%s: %d images, the by-value table holds %d", who, batch->n, WSOVOD_INPUT_MAX_IMAGES);
    return WSOVOD_ERR_UNSUPPORTED;
  }
  return resample_windows(who, *batch, tables, table_ints, scratch, scratch_bytes, canvas, Hp, Wp, stream);
}

long long wsovod_transform_proposals_workspace_bytes(int total_rows) {
  if (total_rows < 0) return 0;
  const long long n = total_rows, t = table_entries(n);
  return t * 8 + t * 4 + n * 16 + n * 4 + 16;  // keys, rows, mapped (its start rounded up to 16), slot
}

int wsovod_transform_proposals(const wsovod_proposal_batch* batch, const float* boxes, const float* logits, int total_rows,
                               int topk, void* workspace, long long workspace_bytes, float* out_boxes, float* out_logits,
                               int* out_count, wsovod_stream_t stream) {
  static const char who[] = "wsovod_transform_proposals";
  WS_CHECK_ARG(batch, "%s: null image table", who);
  if (batch->n > WSOVOD_INPUT_MAX_IMAGES) {
    wsovod::set_error("%s: %d images, the by-value table holds %d", who, batch->n, WSOVOD_INPUT_MAX_IMAGES);
    return WSOVOD_ERR_UNSUPPORTED;
  }
  wsovod_proposal_window_batch b = {};
  b.n = batch->n;
  for (int g = 0; g < batch->n; ++g) {
    const wsovod_proposal_image& d = batch->img[g];
    b.img[g] = {d.start, d.count, d.sx, d.sy, d.flip, d.flip_w, d.clip_w, d.clip_h, 0, 0.0f, 0.0f, 0};
  }
  return proposal_windows(who, b, boxes, logits, total_rows, topk, workspace, workspace_bytes, out_boxes, out_logits, out_count,
                          stream);
}

int wsovod_transform_proposals_win(const wsovod_proposal_window_batch* batch, const float* boxes, const float* logits,
                                   int total_rows, int topk, void* workspace, long long workspace_bytes, float* out_boxes,
                                   float* out_logits, int* out_count, wsovod_stream_t stream) {
  static const char who[] = "wsovod_transform_proposals_win";
  WS_CHECK_ARG(batch, "%s: null image table", who);
  if (batch->n > WSOVOD_INPUT_MAX_IMAGES) {
    wsovod::set_error("%s: %d images, the by-value table holds %d", who, batch->n, WSOVOD_INPUT_MAX_IMAGES);
    return WSOVOD_ERR_UNSUPPORTED;
  }
  return proposal_windows(who, *batch, boxes, logits, total_rows, topk, workspace, workspace_bytes, out_boxes, out_logits,
                          out_count, stream);
}

}  // extern "C"
