// Pieces shared by the GEMM / implicit-GEMM kernels (gemm.hip: generic tiles; gemm8.hip: the 8-phase 256x256 tile).
#pragma once
#include <limits.h>

#include "common.h"

namespace wsovod_gemm {

struct GemmArgs {
  const char* A;
  const char* B;
  long long lda, ldb;  // elements
  int M, N, K;
  void* C;
  long long ldc;
  int dtype_c;
  void* Ct;
  long long ldct;
  int dtype_ct;
  float alpha;
  const float* row_scale;
  const float* bias;
  const void* residual;
  long long ldr;
  int dtype_r;
  int relu;
  float dropout_p;
  unsigned long long seed;
  const unsigned long long* seed_add;  // optional device scalar added to `seed` (a step counter kept on the device)
  const int* row_group;
  const float* group_add;
  long long ld_ga;
  const void* mask_src;
  long long ldm;
  int dtype_m;
  float mask_scale;
  int accumulate;
  // implicit-GEMM convolution geometry
  int H, W, Cin, Ho, Wo, KH, KW, stride, pad, dil;
  int pool;  // conv3x3_c64 only: 2 = MaxPool2d(2, 2) fused into the epilogue, C is the pooled map
  // split-K (gemm8.hip, plain GEMMs with few output tiles): the grid is ksplit copies of the tile grid, copy z reduces
  // K-steps [z*slice_steps, (z+1)*slice_steps) and stores its raw fp32 sums to partial[z][M][partial_ld]; a finalize
  // kernel adds the copies and applies the epilogue
  int ksplit, slice_steps;
  float* partial;
  long long partial_ld;
  long long a_bytes;  // conv: byte size of the NHWC input (must be < 2^31)
  long long a_plane;  // plain GEMM on a PLANAR bf16x2 A (WSOVOD_BF16X2P): bytes from the hi plane to the lo plane, 0 = interleaved
  int tiles_m, tiles_n;
  int m_base;  // gemm_nt_kernel: first output row of this launch (a launch may cover rows [m_base, M) only: tail launches)
  int group_m;  // tile-order group height (see the XCD remap in the kernel)
  // conv: optional second input contracted 1x1 / stride 1 after the KH*KW*Cin main K range (fused projection shortcut)
  const char* A2;
  int Cin2;
  long long a2_bytes;
};

// The branch-batched conv (wsovod_gemm_conv_branches): the tile grid is n_branch stacks of tiles_per_branch row tiles, stack
// b convolving with dil[b] / pad[b] on input A + b * a_branch_bytes (0: one shared input) into C + b * c_branch_bytes; M and
// a_bytes are ONE branch's, so no tile straddles two branches
struct GemmBrArgs : GemmArgs {
  int tiles_per_branch;
  int dil[4], pad[4];
  long long a_branch_bytes, c_branch_bytes;
};
// wsovod_gemm_conv_branches_ex: the same with a residual (d->residual) at residual + b * r_branch_bytes (0: ONE shared
// (N, Ho, Wo, Cout) residual added to every branch) and 1x1 filters next to 3x3
struct GemmBrExArgs : GemmBrArgs {
  long long r_branch_bytes;
};

// ---- host side: what every front does before it picks a kernel

// Tile-order group height (the XCD remap of the kernels walks groups of group_m row tiles).  What has to share L2 is the set
// of workgroups an XCD runs AT THE SAME TIME (32 CUs x 1 workgroup), not its whole run of tiles: group_m x (32 / group_m) of
// them should be near-square, hence the cap of the one-workgroup-per-CU 256x256 tiles (INT_MAX: the square root of the run).
// Measured on the fc1 forward shape (16384 x 4096 x 25088): group 2/4/8/11/16/32 -> 1345/1350/1322/1298/1292/1260 TFLOP/s.
inline int tile_group_height(int tiles_m, int tiles_n, int cap) {
  const int run = std::max(1, tiles_m * tiles_n / 8);  // tiles per XCD
  int g = 1;
  while ((g + 1) * (g + 1) <= run) ++g;
  return std::max(1, std::min(std::min(g, cap), tiles_m));
}

// The descriptor's fields as the kernels take them.  A value is `slots` operand elements wide (bf16x2, f16mx: 2), so the
// leading dimensions and K are counted in slots; a planar A row holds lda bf16 values, the interleaved row slots * lda
inline void fill_gemm_args(GemmArgs& a, const wsovod_gemm_desc& d, int slots) {
  memset(&a, 0, sizeof(a));
  a.A = (const char*)d.A, a.B = (const char*)d.B;
  a.a_plane = d.a_plane_bytes, a.lda = d.a_plane_bytes ? d.lda : d.lda * slots, a.ldb = d.ldb * slots;
  a.M = d.M, a.N = d.N, a.K = d.K * slots;
  a.C = d.C, a.ldc = d.ldc, a.dtype_c = d.dtype_c;
  a.Ct = d.Ct, a.ldct = d.ldct, a.dtype_ct = d.dtype_ct;
  a.alpha = d.alpha, a.row_scale = d.row_scale, a.bias = d.bias;
  a.residual = d.residual, a.ldr = d.ldr, a.dtype_r = d.dtype_r;
  a.relu = d.relu, a.dropout_p = d.dropout_p, a.seed = d.dropout_seed, a.seed_add = d.dropout_seed_add;
  a.row_group = d.row_group, a.group_add = d.group_add, a.ld_ga = d.ld_ga;
  a.mask_src = d.mask_src, a.ldm = d.ldm, a.dtype_m = d.dtype_m, a.mask_scale = d.mask_scale;
  a.accumulate = d.accumulate;
}

// The implicit-GEMM conv form: the checks every conv kernel relies on, then the geometry and the operands' byte sizes
// (slots of slot_bytes each per value; Cin, Cin2 multiples of cin_multiple values).  border_in_limit: the 2 GiB limit of the
// input counts the pad border in front of it.  The f16mx front asks for that; the bf16 / bf16x2 / fp32 front does not (its lean
// 8-wavefront tile tests the border itself and leaves such an input to the general form).  The two fronts were found to
// differ in this and still do: the flag keeps the difference at the call sites.  `who`: the entry's name in the messages.
inline int check_and_fill_conv(GemmArgs& a, const wsovod_gemm_desc& d, int slots, int slot_bytes, int cin_multiple,
                               bool border_in_limit, const char* who) {
  const wsovod_conv_geom& g = d.geom;
  WS_CHECK_ARG(g.Cin > 0 && g.Cin % cin_multiple == 0, "%s(conv): Cin=%d must be a multiple of %d", who, g.Cin, cin_multiple);
  WS_CHECK_ARG(!d.A2 || (d.Cin2 > 0 && d.Cin2 % cin_multiple == 0 && ((uintptr_t)d.A2 & 15) == 0),
               "%s(conv): the fused shortcut input needs Cin2 (%d) a multiple of %d and 16-byte alignment", who, d.Cin2, cin_multiple);
  WS_CHECK_ARG(d.K == g.KH * g.KW * g.Cin + (d.A2 ? d.Cin2 : 0), "%s(conv): K=%d != KH*KW*Cin (+ Cin2)", who, d.K);
  WS_CHECK_ARG(g.KH * g.KW <= 32, "%s(conv): filters of more than 32 taps are not supported (per-tap validity mask)", who);
  WS_CHECK_ARG((long long)d.M == (long long)g.n_img * g.Ho * g.Wo, "%s(conv): M=%d != n_img*Ho*Wo", who, d.M);
  WS_CHECK_ARG(g.stride >= 1 && g.dil >= 1 && g.pad >= 0, "%s(conv): bad stride/dil/pad", who);
  const int vbytes = slots * slot_bytes;
  a.H = g.H, a.W = g.W, a.Cin = g.Cin * slots, a.Ho = g.Ho, a.Wo = g.Wo;
  a.KH = g.KH, a.KW = g.KW, a.stride = g.stride, a.pad = g.pad, a.dil = g.dil, a.pool = g.pool;
  a.a_bytes = (long long)g.n_img * g.H * g.W * g.Cin * vbytes;
  if (d.A2) {
    a.A2 = (const char*)d.A2;
    a.Cin2 = d.Cin2 * slots;
    a.a2_bytes = (long long)g.n_img * g.Ho * g.Wo * d.Cin2 * vbytes;
    WS_CHECK_ARG(a.a2_bytes < (1ll << 31), "%s(conv): fused shortcut input exceeds the 2 GiB buffer-addressing limit", who);
  }
  const long long border = border_in_limit ? (long long)(g.pad * g.W + g.pad) * g.Cin * vbytes : 0;
  WS_CHECK_ARG(a.a_bytes + border < (1ll << 31), "%s(conv): input of %lld bytes exceeds the 2 GiB buffer-addressing limit", who,
               a.a_bytes);
  return WSOVOD_OK;
}

// The branch-batched conv (2-byte slots): the 2 GiB limit is kept for the WHOLE n_branch * N operand, with the largest
// branch's border in front.  `who`: wsovod_gemm_conv_branches / wsovod_gemm_f16mx_conv_branches
inline int check_branch_limit(const GemmArgs& a, const wsovod_conv_branches& br, const char* who) {
  int pmax = 0;
  for (int b = 0; b < br.n_branch; ++b) pmax = std::max(pmax, br.pad[b]);
  WS_CHECK_ARG(a.a_bytes * (br.shared_input ? 1 : br.n_branch) + (long long)(pmax * a.W + pmax) * a.Cin * 2 < (1ll << 31) &&
                   (long long)a.M * br.n_branch < (1ll << 31),
               "%s: the n_branch * N input exceeds the 2 GiB buffer-addressing limit", who);
  return WSOVOD_OK;
}

template <typename T>
struct Traits;
template <>
struct Traits<float> {
  static constexpr int EPC = 4;   // elements per 16-byte chunk
  static constexpr int BKE = 32;  // elements per K-step (128 B)
};
template <>
struct Traits<bf16_t> {
  static constexpr int EPC = 8;
  static constexpr int BKE = 64;
};

__device__ __forceinline__ int lds_off(int row, int chunk) {
  return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
}

// ---- bf16x2 (include/wsovod_hip.h: WSOVOD_BF16X2): value k of a row sits at bf16 index x2_pos(k) (hi) and
// x2_pos(k) + 32 (lo) of the row's 2 * ld bf16 slots
__device__ __forceinline__ long long x2_pos(int k) { return ((long long)(k >> 5) << 6) | (k & 31); }
__device__ __forceinline__ bf16_t x2_lo(float v, bf16_t hi) {
  const float h = (float)hi;
  return (bf16_t)(__builtin_isinf(h) ? 0.f : v - h);  // an infinite value stays infinite (inf - inf would store a NaN)
}

// element (m, n) of a row-major matrix with leading dimension ld (values) in any of the three dtypes
__device__ __forceinline__ float load_as_f32(const void* p, long long m, long long ld, int n, int dtype) {
  if (dtype == WSOVOD_BF16) return (float)((const bf16_t*)p)[m * ld + n];
  if (dtype == WSOVOD_BF16X2) {
    const bf16_t* q = (const bf16_t*)p + 2 * m * ld + x2_pos(n);
    return (float)q[0] + (float)q[32];
  }
  return ((const float*)p)[m * ld + n];
}
__device__ __forceinline__ void store_from_f32(void* p, long long m, long long ld, int n, int dtype, float v) {
  if (dtype == WSOVOD_BF16) {
    ((bf16_t*)p)[m * ld + n] = (bf16_t)v;
  } else if (dtype == WSOVOD_BF16X2) {
    bf16_t* q = (bf16_t*)p + 2 * m * ld + x2_pos(n);
    const bf16_t hi = (bf16_t)v;
    q[0] = hi;
    q[32] = x2_lo(v, hi);
  } else {
    ((float*)p)[m * ld + n] = v;
  }
}
// 4 consecutive values n .. n+3 (n a multiple of 4; rows 8-byte (bf16, bf16x2) / 16-byte (fp32) aligned)
__device__ __forceinline__ f32x4 load4_as_f32(const void* p, long long m, long long ld, int n, int dtype) {
  if (dtype == WSOVOD_BF16) {
    const bf16x4 r = *(const bf16x4*)((const bf16_t*)p + m * ld + n);
    return f32x4{(float)r[0], (float)r[1], (float)r[2], (float)r[3]};
  }
  if (dtype == WSOVOD_BF16X2) {
    const bf16_t* q = (const bf16_t*)p + 2 * m * ld + x2_pos(n);
    const bf16x4 h = *(const bf16x4*)q, l = *(const bf16x4*)(q + 32);
    return f32x4{(float)h[0] + (float)l[0], (float)h[1] + (float)l[1], (float)h[2] + (float)l[2], (float)h[3] + (float)l[3]};
  }
  return *(const f32x4*)((const float*)p + m * ld + n);
}
__device__ __forceinline__ void store4_from_f32(void* p, long long m, long long ld, int n, int dtype, const f32x4 v) {
  if (dtype == WSOVOD_BF16) {
    *(bf16x4*)((bf16_t*)p + m * ld + n) = bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
  } else if (dtype == WSOVOD_BF16X2) {
    bf16_t* q = (bf16_t*)p + 2 * m * ld + x2_pos(n);
    const bf16x4 h = bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
    *(bf16x4*)q = h;
    *(bf16x4*)(q + 32) = bf16x4{x2_lo(v[0], h[0]), x2_lo(v[1], h[1]), x2_lo(v[2], h[2]), x2_lo(v[3], h[3])};
  } else {
    *(f32x4*)((float*)p + m * ld + n) = v;
  }
}
// true when 4-value groups of rows of `p` can move as the vector accesses above
__device__ __forceinline__ bool vec4_ok(const void* p, long long ld, int dtype) {
  if (dtype == WSOVOD_F32) return (ld & 3) == 0 && ((uintptr_t)p & 15) == 0;
  if (dtype == WSOVOD_BF16) return (ld & 3) == 0 && ((uintptr_t)p & 7) == 0;
  return (ld & 31) == 0 && ((uintptr_t)p & 15) == 0;  // bf16x2: whole 32-value groups per row
}

// the dropout seed of this launch: the host part plus, when given, the device-resident step term (a captured HIP graph
// replays with the same kernel arguments: the part of the seed that changes per step lives in memory)
#define WS_DROPOUT_SEED(p) ((p).seed_add ? (p).seed + *(p).seed_add : (p).seed)

// Counter-based, stateless dropout mask on (seed, m, n): ONE splitmix64 value per quad of consecutive columns
// (n & ~3 .. n | 3 of row m), 16 of its bits per element: keep iff bits >= p * 2^16 (round 5: a 64-bit hash per element was
// ~40 VALU instructions each, ~0.18 ms of the step in the FC epilogues; p is honoured to 2^-16, 0.5 exactly)
__device__ __forceinline__ unsigned long long dropout_quad(unsigned long long seed, long long m, int N, int nb) {
  const unsigned long long ctr = (unsigned long long)m * (unsigned long long)((N + 3) >> 2) + (unsigned long long)(nb >> 2);
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (ctr + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ unsigned dropout_threshold(float p) { return (unsigned)(p * 65536.0f + 0.5f); }
__device__ __forceinline__ bool dropout_keep(unsigned long long z, int r, unsigned thr) {
  return (unsigned)((z >> (16 * r)) & 0xFFFFull) >= thr;
}

// The epilogue chain of the GEMM kernels for 4 consecutive columns nb..nb+3 of row m (v = raw sums), stores included:
// used by the split-K finalize kernels (the tile kernels carry vectorised copies of the same chain).
__device__ __forceinline__ void epilogue_store4(const GemmArgs& p, int m, int nb, const float (&v)[4]) {
  const float keep_scale = p.dropout_p > 0.f ? 1.0f / (1.0f - p.dropout_p) : 1.0f;
  const float rs = p.row_scale ? p.row_scale[m] : 1.f;
  const unsigned long long dz = p.dropout_p > 0.f ? dropout_quad(WS_DROPOUT_SEED(p), m, p.N, nb) : 0ull;
  const unsigned dthr = dropout_threshold(p.dropout_p);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = nb + r;
    if (n >= p.N) continue;
    float x = v[r] * p.alpha;
    if (p.row_scale) x *= rs;
    if (p.bias) x += p.bias[n];
    if (p.residual) x += load_as_f32(p.residual, m, p.ldr, n, p.dtype_r);
    if (p.relu) x = fmaxf(x, 0.f);
    if (p.dropout_p > 0.f) x = dropout_keep(dz, r, dthr) ? x * keep_scale : 0.f;
    if (p.group_add) x += p.group_add[(long long)p.row_group[m] * p.ld_ga + n];
    if (p.mask_src) x = load_as_f32(p.mask_src, m, p.ldm, n, p.dtype_m) > 0.f ? x * p.mask_scale : 0.f;
    if (p.C && p.accumulate) x += ((float*)p.C)[(long long)m * p.ldc + n];
    if (p.C) store_from_f32(p.C, m, p.ldc, n, p.dtype_c, x);
    if (p.Ct) store_from_f32(p.Ct, n, p.ldct, m, p.dtype_ct, x);
  }
}

// gemm8.hip: bf16 256x256 tile, 8 wavefronts in two staggered groups (see the file header).
// x3: bf16x2 operands (three-MFMA products); merged: the two-phase form of the K-step (tile_hint 2256256)
int launch_gemm256_8ph(const GemmArgs& a, bool conv, hipStream_t s, double flops, double bytes, bool allow_split = false,
                       bool x3 = false, bool merged = false);
// the lean two-phase bf16x2 conv tile over n_branch dilations in ONE launch (a.M, a.a_bytes: one branch's)
int launch_gemm256_8ph_branches(const GemmArgs& a, int n_branch, const int* dil, const int* pad, bool shared_input,
                                hipStream_t s, double flops, double bytes);
// the same with the residual epilogue (a.residual: one branch's rows, or with shared_residual ONE map for every branch)
int launch_gemm256_8ph_branches_ex(const GemmArgs& a, int n_branch, const int* dil, const int* pad, bool shared_input,
                                   bool shared_residual, hipStream_t s, double flops, double bytes);

}  // namespace wsovod_gemm
