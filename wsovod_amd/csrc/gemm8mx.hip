// Round 6 (MODEL.HIP.PRECISION = "parity_mx"): the forward contractions of the big layers -- the res4 / res5 implicit-GEMM
// convolutions and the two FC layers of the box head -- on gfx950's block-scaled matrix instruction: the two cross terms of the
// three-product forward (hi*lo + lo*hi, 2^-12 of a product when hi is an fp16 rounding) as ONE
// v_mfma_scale_f32_32x32x64_f8f6f4 on e4m3 planes, hi*hi as two v_mfma_f32_32x32x16_f16: per 32x32 output tile and 32 values of
// K 128 matrix-pipe cycles where the bf16x2 form (gemm8.hip) spends 192.
//
// Operand format "f16mx" (f16mx.h; the same 4 bytes per value and row stride as bf16x2): a row is groups of 32 values = 128
// bytes [32 x fp16 hi | 32 x e4m3 q | 32 x e4m3 ql], q = e4m3(x 2^-s), ql = e4m3((x - hi) 2^-(s - 11)) -- |x - hi| is at most
// half an fp16 ulp, so the lo plane's scale is TIED 11 binades below the q plane's and one exponent serves both.  Scales are
// LOOP CONSTANTS of the kernel: activations (A) carry none (s = 0, written by the producing epilogue without a row maximum),
// weights (B) one E8M0 byte per row (or per row segment) in a side array.  e4m3's own exponent carries the dynamic range
// inside a row.  Numerics gate: profiles/r06_mx_gate.md (tools/mx_emulation.py, "THE BUILD": logits 2.1e-4 from the oracle).
//
// The kernel is the 8-wavefront 256x256 two-phase staggered tile of gemm8.hip with
//   * 32-row MFMA tiles: lane (r = lane & 31, h = lane >> 5) reads, per tile and K-step, 32 bytes of the hi plane (chunks 2h,
//     2h+1: fp16 values 16h .. 16h+15, the two 32x32x16 products) and 32 bytes of an fp8 plane -- A: q for h = 0, ql for h = 1;
//     B: ql for h = 0, q for h = 1 -- so the scaled MFMA's K halves are q_a*ql_b and ql_a*q_b.  Same 128-byte LDS rows, same
//     DMA and XOR swizzle as the bf16x2 tile.  The two 16-byte pieces of an fp8 operand are read into FIXED adjacent physical
//     registers (the instruction takes 8 consecutive VGPRs; through allocator-chosen registers hipcc assembled them with
//     v_movs, kept a second copy alive and spilled);
//   * a RING of three K-steps for A and B refilled right after its only reads: every LDS-DMA piece is requested two K-steps
//     (three to four phases) before its use, four pieces in each phase; one counted wait per K-step.  With the bf16x2 tile's
//     schedule (one K-step ahead, 6 + 2 pieces) the 512-cycle phases of this format waited on memory: 663 -> 714 TFLOP/s on
//     fc1, matrix pipe 78 -> 90 % busy (tools/mx_phases.py, tools/mx_abl_pmc.sh); what is left is the clock under the power
//     limit (1.45 GHz with fragment reads + DMA, 2.2 GHz on the bare MFMA loop);
//   * B rows permuted at staging so that a lane owns 16 CONSECUTIVE output columns per tile (32x32 accumulator layout:
//     row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)): the epilogue writes 64 bytes per lane and row, also as f16mx;
//   * CONV: the implicit-GEMM gather of gemm8.hip's lean form (per-lane pixel offset + tap validity bits, the tap's
//     displacement as the scalar offset, the fused 1x1 projection shortcut as extra K-steps on a second input), the offsets of
//     the K-step requested next computed under the products of phase B.
// Replaces (opt-in): roi_heads/box_head.py:60-75 (fc1 / fc2 forward, F.linear) and backbone/resnet_wsl.py:94-110 (the conv +
// FrozenBN + shortcut + ReLU of the res4 / res5 BasicBlocks) for the "parity_mx" precision.
#include "gemm_common.h"
#include "f16mx.h"

#include <stdlib.h>

#include <algorithm>
#include <type_traits>

namespace wsovod_gemm {
namespace {

using namespace wsovod_mx;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef int i32x8 __attribute__((ext_vector_type(8)));

struct MxArgs {
  GemmArgs g;               // (K, lda, ldb, Cin, Cin2 in 2-byte slots: a value is two slots, a K-step 64 slots = 32 values)
  const unsigned char* sa;  // [M][nseg_a] E8M0 bytes of the A rows; NULL = unit scale (activations)
  const unsigned char* sb;  // [N][nseg_b]
  int nseg_a, nseg_b;       // equal K segments per row
  void* c_bf16;             // optional plain bf16 copy of C (the operand of the NEXT layer's weight gradient, the mask source)
  long long ld_cb;
  float* dbg;               // (-DMX_STAMPS builds, tools/mx_phases.py) 2 x 16 tick sums
};

// The branch-batched conv (wsovod_gemm_f16mx_conv_branches): the tile grid is n_branch stacks of tiles_per_branch row tiles,
// stack b convolving with dil[b] / pad[b] on input A + b * a_branch_bytes (0: one shared input) into C + b * c_branch_bytes;
// g.M, g.a_bytes are ONE branch's, so a tile never straddles two branches
struct MxBrArgs : MxArgs {
  int tiles_per_branch;
  int dil[4], pad[4];
  long long a_branch_bytes, c_branch_bytes;
};
// wsovod_gemm_f16mx_conv_branches_ex: the same with a residual at g.residual + b * r_branch_bytes (0: ONE shared (N, Ho, Wo,
// Cout) residual added to every branch) and 1x1 filters next to 3x3
struct MxBrExArgs : MxBrArgs {
  long long r_branch_bytes;
};

template <int OFF>
__device__ __forceinline__ void mx_read(u32x4& dst, unsigned addr) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
#endif
}

__device__ __forceinline__ i32x8 mx_cat(const u32x4 a, const u32x4 b) {
  return i32x8{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b[0], (int)b[1], (int)b[2], (int)b[3]};
}

#include "gemm8mx_kernel.h"
#define WSOVOD_CONV_BRANCHES 1
#include "gemm8mx_kernel.h"
#define WSOVOD_CONV_BRANCHES_EX 1
#include "gemm8mx_kernel.h"
#undef WSOVOD_CONV_BRANCHES_EX
#undef WSOVOD_CONV_BRANCHES

// split-K finalize: C[m][n] = epilogue(sum over the K slices) for 4 consecutive columns per thread -- the same chain and the
// same output formats as the tile kernel's epilogue
__global__ __launch_bounds__(256) void mx_splitk_finalize_kernel(const MxArgs q) {
#if defined(__HIP_DEVICE_COMPILE__)
  const GemmArgs& p = q.g;
  const int n4 = p.N >> 2;  // (launcher: N a multiple of 4)
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int rows = p.M - p.m_base;
  if (idx >= (long long)rows * n4) return;
  const int mr = (int)(idx / n4), nb = (int)(idx - (long long)mr * n4) * 4, m = p.m_base + mr;
  f32x4 x = {0.f, 0.f, 0.f, 0.f};
  for (int z = 0; z < p.ksplit; ++z) x += *(const f32x4*)(p.partial + ((long long)z * rows + mr) * p.partial_ld + nb);
  x = x * p.alpha;
  if (p.bias) x += *(const f32x4*)(p.bias + nb);
  if (p.residual) {
    if (p.dtype_r == WSOVOD_F16MX) x += mx_load4_unit((const char*)p.residual + (long long)m * p.ldr * 4, nb);
    else x += load4_as_f32(p.residual, m, p.ldr, nb, p.dtype_r);
  }
  const float lo = p.relu ? 0.f : -__builtin_inff();
  x = f32x4{fmaxf(x[0], lo), fmaxf(x[1], lo), fmaxf(x[2], lo), fmaxf(x[3], lo)};
  if (p.dropout_p > 0.f) {
    const float keep_scale = 1.0f / (1.0f - p.dropout_p);
    const unsigned long long dz = dropout_quad(WS_DROPOUT_SEED(p), m, p.N, nb);
    const unsigned dthr = dropout_threshold(p.dropout_p);
#pragma unroll
    for (int r = 0; r < 4; ++r) x[r] = dropout_keep(dz, r, dthr) ? x[r] * keep_scale : 0.f;
  }
  if (p.dtype_c == WSOVOD_F16MX) mx_store4_unit((char*)p.C + (long long)m * p.ldc * 4, nb, x);
  else store4_from_f32(p.C, m, p.ldc, nb, p.dtype_c, x);
  if (q.c_bf16)
    *(bf16x4*)((bf16_t*)q.c_bf16 + (long long)m * q.ld_cb + nb) = bf16x4{(bf16_t)x[0], (bf16_t)x[1], (bf16_t)x[2], (bf16_t)x[3]};
#endif
}

// ---- plane conversions between the two parity formats (the maps that cross from the bf16x2 layers to the f16mx ones)
__global__ __launch_bounds__(256) void mx_from_x2_kernel(const bf16_t* __restrict__ src, char* __restrict__ dst, long long ngroups) {
#if defined(__HIP_DEVICE_COMPILE__)
  // a thread per 8 values of a 32-value group: bf16x2 group = [32 hi | 32 lo] bf16, same 128 bytes as the f16mx group
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long grp = t >> 2;
  if (grp >= ngroups) return;
  const int w = (int)(t & 3) * 8;
  const bf16_t* s = src + grp * 64 + w;
  const bf16x8 h = *(const bf16x8*)s, l = *(const bf16x8*)(s + 32);
  f16x4 h0, h1;
  int q0, q1, l0, l1;
  mx_enc4_unit(f32x4{(float)h[0] + (float)l[0], (float)h[1] + (float)l[1], (float)h[2] + (float)l[2], (float)h[3] + (float)l[3]}, h0, q0, l0);
  mx_enc4_unit(f32x4{(float)h[4] + (float)l[4], (float)h[5] + (float)l[5], (float)h[6] + (float)l[6], (float)h[7] + (float)l[7]}, h1, q1, l1);
  char* d = dst + grp * 128;
  *(f16x8*)(d + 2 * w) = f16x8{h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
  *(i32x2*)(d + 64 + w) = i32x2{q0, q1};
  *(i32x2*)(d + 96 + w) = i32x2{l0, l1};
#endif
}

// ---- encoder: fp32 (rows, cols) -> f16mx carrier + one scale byte per (row, segment); a workgroup per (row, segment):
// pass 1 the segment's largest |fp16(x)| (exponent field), pass 2 the planes.  scales == NULL: the unit-scale form
__global__ __launch_bounds__(256) void mx_encode_kernel(const float* __restrict__ src, long long ld_src, int rows, int cols,
                                                        int nseg, unsigned char* __restrict__ dst, long long ld_dst_bytes,
                                                        unsigned char* __restrict__ scales,
                                                        const unsigned char* __restrict__ tscale = nullptr) {
#if defined(__HIP_DEVICE_COMPILE__)
  __shared__ unsigned red[4];
  const int r = blockIdx.x / nseg, sg = blockIdx.x - r * nseg;
  const int seg_cols = cols / nseg, c0 = sg * seg_cols;
  const float* s = src + (long long)r * ld_src + c0;
  int sexp = 0;  // q scale 2^sexp; ql scale 2^(sexp - 11)
  if (tscale) {  // one scale for the whole tensor, chosen by the caller
    sexp = (int)*tscale - 127;
    if (threadIdx.x == 0) scales[(long long)r * nseg + sg] = *tscale;
  } else if (scales) {
    unsigned mx = 0;
    for (int e = threadIdx.x * 4; e < seg_cols; e += 256 * 4) {
      const f32x4 t = *(const f32x4*)(s + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) mx = max(mx, (unsigned)(__builtin_bit_cast(unsigned short, (_Float16)t[j]) & 0x7fffu));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = max(max(red[0], red[1]), max(red[2], red[3]));
    const int ef = min((int)(mx >> 10), 30);  // fp16 exponent field of the largest |hi| (31 = inf / nan: treated as 30)
    sexp = (ef == 0 ? -14 : ef - 15) - 7;
    if (threadIdx.x == 0) scales[(long long)r * nseg + sg] = (unsigned char)(sexp + 127);
  }
  const float inv_q = __builtin_ldexpf(1.0f, -sexp), inv_l = __builtin_ldexpf(1.0f, -(sexp - 11));
  // one thread per 8 values: 16 B of hi, 8 B of q, 8 B of ql
  unsigned char* drow = dst + (long long)r * ld_dst_bytes;
  for (int e = threadIdx.x * 8; e < seg_cols; e += 256 * 8) {
    const int c = c0 + e;
    f16x4 h0, h1;
    int q0, q1, l0, l1;
    mx_enc4(*(const f32x4*)(s + e), inv_q, inv_l, h0, q0, l0);
    mx_enc4(*(const f32x4*)(s + e + 4), inv_q, inv_l, h1, q1, l1);
    unsigned char* d = drow + mx_group(c);
    const int w = c & 31;  // position inside the group of 32 (a multiple of 8)
    *(f16x8*)(d + 2 * w) = f16x8{h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
    *(i32x2*)(d + 64 + w) = i32x2{q0, q1};
    *(i32x2*)(d + 96 + w) = i32x2{l0, l1};
  }
#endif
}

}  // namespace
}  // namespace wsovod_gemm

using namespace wsovod_gemm;

extern "C" int wsovod_f16mx_encode(const float* src, long long ld_src, int rows, int cols, int nseg, void* dst, long long ld_dst,
                                   unsigned char* scales, wsovod_stream_t stream) {
  WS_CHECK_ARG(rows >= 0 && cols >= 0 && nseg >= 1 && cols % (32 * nseg) == 0,
               "wsovod_f16mx_encode: cols=%d must be a multiple of 32 * nseg (%d)", cols, nseg);
  if (rows == 0 || cols == 0) return WSOVOD_OK;
  WS_CHECK_ARG(src && dst && ld_src >= cols && ld_src % 4 == 0 && ld_dst >= cols && ld_dst % 4 == 0 &&
                   (((uintptr_t)dst | (uintptr_t)src) & 15) == 0,
               "wsovod_f16mx_encode: bad pointer / leading dimension");
  static int slot = wsovod::prof_slot("f16mx_encode");
  hipStream_t s = (hipStream_t)stream;
  wsovod::ProfScope prof(slot, s, 0.0, (double)rows * cols * 8.0);
  hipLaunchKernelGGL(mx_encode_kernel, dim3((unsigned)((long long)rows * nseg)), dim3(256), 0, s, src, ld_src, rows, cols, nseg,
                     (unsigned char*)dst, ld_dst * 4, scales, (const unsigned char*)nullptr);
  WS_CHECK_LAUNCH("wsovod_f16mx_encode");
  return WSOVOD_OK;
}

extern "C" int wsovod_f16mx_encode_with(const float* src, long long ld_src, int rows, int cols, void* dst, long long ld_dst,
                                        unsigned char* scales, const unsigned char* tensor_scale, wsovod_stream_t stream) {
  WS_CHECK_ARG(rows >= 0 && cols >= 0 && cols % 32 == 0, "wsovod_f16mx_encode_with: cols=%d must be a multiple of 32", cols);
  if (rows == 0 || cols == 0) return WSOVOD_OK;
  WS_CHECK_ARG(src && dst && scales && tensor_scale && ld_src >= cols && ld_src % 4 == 0 && ld_dst >= cols && ld_dst % 4 == 0 &&
                   (((uintptr_t)dst | (uintptr_t)src) & 15) == 0,
               "wsovod_f16mx_encode_with: bad pointer / leading dimension");
  static int slot = wsovod::prof_slot("f16mx_encode");
  hipStream_t s = (hipStream_t)stream;
  wsovod::ProfScope prof(slot, s, 0.0, (double)rows * cols * 8.0);
  hipLaunchKernelGGL(mx_encode_kernel, dim3((unsigned)rows), dim3(256), 0, s, src, ld_src, rows, cols, 1, (unsigned char*)dst,
                     ld_dst * 4, scales, tensor_scale);
  WS_CHECK_LAUNCH("wsovod_f16mx_encode_with");
  return WSOVOD_OK;
}

extern "C" int wsovod_f16mx_from_bf16x2(const void* src, void* dst, long long n, wsovod_stream_t stream) {
  WS_CHECK_ARG(n >= 0 && n % 32 == 0, "wsovod_f16mx_from_bf16x2: n=%lld must be whole 32-value groups", n);
  if (n == 0) return WSOVOD_OK;
  WS_CHECK_ARG(src && dst && (((uintptr_t)dst | (uintptr_t)src) & 15) == 0, "wsovod_f16mx_from_bf16x2: bad pointer");
  static int slot = wsovod::prof_slot("f16mx_from_bf16x2");
  hipStream_t s = (hipStream_t)stream;
  wsovod::ProfScope prof(slot, s, 0.0, (double)n * 8.0);
  const long long threads = n / 8;
  hipLaunchKernelGGL(mx_from_x2_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, (const bf16_t*)src, (char*)dst, n / 32);
  WS_CHECK_LAUNCH("wsovod_f16mx_from_bf16x2");
  return WSOVOD_OK;
}

// br != NULL: the branch-batched conv of wsovod_gemm_f16mx_conv_branches (d->M, geom.n_img: ONE branch's); ex != NULL: its
// _ex form (residual epilogue, *ex = the residual is ONE map shared by the branches; 1x1 filters next to 3x3)
static int gemm_f16mx_impl(const wsovod_gemm_desc* d, const unsigned char* a_scale, int a_segments,
                           const unsigned char* b_scale, int b_segments, void* c_bf16, long long ld_c_bf16,
                           const wsovod_conv_branches* br, wsovod_stream_t stream, const int* ex = nullptr) {
  WS_CHECK_ARG(d && b_scale, "wsovod_gemm_f16mx: null descriptor / weight scale array");
  wsovod_gemm_desc d1x1;
  wsovod_conv_branches br1x1;
  if (br && ex) {
    WS_CHECK_ARG(br->n_branch >= 1 && br->n_branch <= 4, "wsovod_gemm_f16mx_conv_branches_ex: n_branch=%d must be 1 - 4", br->n_branch);
    WS_CHECK_ARG(d->conv && !d->A2 && d->dropout_p == 0.f && !c_bf16 && !a_scale && d->alpha == 1.0f,
                 "wsovod_gemm_f16mx_conv_branches_ex: a conv with the bias + residual + ReLU epilogue (no shortcut, dropout, bf16 copy)");
    const bool k3 = d->geom.KH == 3 && d->geom.KW == 3, k1 = d->geom.KH == 1 && d->geom.KW == 1;
    WS_CHECK_ARG((k3 || k1) && d->geom.stride == 1 && d->geom.Ho == d->geom.H && d->geom.Wo == d->geom.W,
                 "wsovod_gemm_f16mx_conv_branches_ex: 3x3 or 1x1, stride 1, output of the input's size");
    WS_CHECK_ARG(!d->residual || d->dtype_r == WSOVOD_F16MX || d->dtype_r == WSOVOD_BF16X2 || d->dtype_r == WSOVOD_F32,
                 "wsovod_gemm_f16mx_conv_branches_ex: the residual is f16mx, bf16x2 or fp32");
    WS_CHECK_ARG(d->dtype_c == WSOVOD_F16MX || d->dtype_c == WSOVOD_BF16X2 || d->dtype_c == WSOVOD_F32,
                 "wsovod_gemm_f16mx_conv_branches_ex: the output is f16mx, bf16x2 or fp32");
    if (k1) {  // a 1x1 filter has no dilation: every branch runs it at dil 1 / pad 0 on its own rows
      d1x1 = *d;
      br1x1 = *br;
      d1x1.geom.dil = 1;
      d1x1.geom.pad = 0;
      for (int b = 0; b < 4; ++b) br1x1.dil[b] = 1, br1x1.pad[b] = 0;
      d = &d1x1;
      br = &br1x1;
    } else {
      for (int b = 0; b < br->n_branch; ++b)
        WS_CHECK_ARG(br->dil[b] >= 1 && br->pad[b] == br->dil[b], "wsovod_gemm_f16mx_conv_branches_ex: branch %d needs pad == dil >= 1", b);
    }
  } else if (br) {
    WS_CHECK_ARG(br->n_branch >= 1 && br->n_branch <= 4, "wsovod_gemm_f16mx_conv_branches: n_branch=%d must be 1 - 4", br->n_branch);
    WS_CHECK_ARG(d->conv && !d->A2 && !d->residual && d->dropout_p == 0.f && !c_bf16 && !a_scale,
                 "wsovod_gemm_f16mx_conv_branches: a conv with the bias + ReLU epilogue (no shortcut, residual, dropout, bf16 copy)");
    WS_CHECK_ARG(d->geom.KH == 3 && d->geom.KW == 3 && d->geom.stride == 1 && d->geom.Ho == d->geom.H && d->geom.Wo == d->geom.W,
                 "wsovod_gemm_f16mx_conv_branches: 3x3, stride 1, output of the input's size");
    for (int b = 0; b < br->n_branch; ++b)
      WS_CHECK_ARG(br->dil[b] >= 1 && br->pad[b] == br->dil[b], "wsovod_gemm_f16mx_conv_branches: branch %d needs pad == dil >= 1", b);
    WS_CHECK_ARG(d->dtype_c == WSOVOD_F16MX || d->dtype_c == WSOVOD_BF16X2 || d->dtype_c == WSOVOD_F32,
                 "wsovod_gemm_f16mx_conv_branches: the output is f16mx, bf16x2 or fp32");
  }
  WS_CHECK_ARG(d->a_plane_bytes == 0 && (d->conv || !d->A2), "wsovod_gemm_f16mx: interleaved operands; A2 is the conv form's shortcut input");
  WS_CHECK_ARG(d->M >= 0 && d->N >= 0 && d->K > 0 && d->K % 32 == 0 && a_segments >= 1 && b_segments >= 1 &&
                   (d->K / 32) % a_segments == 0 && (d->K / 32) % b_segments == 0,
               "wsovod_gemm_f16mx: K=%d must be whole 32-value groups, split evenly into the operands' scale segments", d->K);
  {
    const int sa = d->K / 32 / a_segments, sb = d->K / 32 / b_segments;
    WS_CHECK_ARG((a_segments == 1 || sa % 6 == 0) && (b_segments == 1 || sb % 6 == 0),
                 "wsovod_gemm_f16mx: a scale segment (%d / %d groups of 32) must be the whole row or a multiple of 6 groups", sa, sb);
  }
  if (d->M == 0 || d->N == 0) return WSOVOD_OK;
  WS_CHECK_ARG(d->A && d->B, "wsovod_gemm_f16mx: null pointer");
  WS_CHECK_ARG(d->ldb % 4 == 0 && d->ldb >= d->K && (((uintptr_t)d->A | (uintptr_t)d->B) & 15) == 0 &&
                   320ll * d->ldb * 4 < (1ll << 31),
               "wsovod_gemm_f16mx: operands must be 16-byte aligned f16mx rows (a tile of weight rows below 2 GiB)");
  WS_CHECK_ARG(d->dropout_p >= 0.f && d->dropout_p < 1.f, "wsovod_gemm_f16mx: dropout_p must be in [0,1)");
  WS_CHECK_ARG(d->C && !d->Ct && !d->row_scale && !d->group_add && !d->mask_src && !d->accumulate,
               "wsovod_gemm_f16mx: the epilogue is alpha / bias / residual / ReLU / dropout");
  WS_CHECK_ARG(d->N % 4 == 0 && (!d->bias || ((uintptr_t)d->bias & 15) == 0) &&
                   (d->dtype_c == WSOVOD_BF16X2 || d->dtype_c == WSOVOD_F16MX
                        ? (d->ldc % 32 == 0 && ((uintptr_t)d->C & 15) == 0 && (d->dtype_c == WSOVOD_BF16X2 || d->N % 16 == 0))
                    : d->dtype_c == WSOVOD_BF16 ? (d->ldc % 4 == 0 && ((uintptr_t)d->C & 7) == 0)
                                                : (d->dtype_c == WSOVOD_F32 && d->ldc % 4 == 0 && ((uintptr_t)d->C & 15) == 0)),
               "wsovod_gemm_f16mx: N must be a multiple of 4 (16 for an f16mx output) and the output rows vector-aligned "
               "(bf16x2 / f16mx: whole 32-value groups)");
  WS_CHECK_ARG(!c_bf16 || (ld_c_bf16 % 8 == 0 && ld_c_bf16 >= d->N && ((uintptr_t)c_bf16 & 15) == 0),
               "wsovod_gemm_f16mx: the bf16 copy needs 16-byte aligned rows");
  WS_CHECK_ARG(!d->residual || (d->dtype_r == WSOVOD_F16MX || d->dtype_r == WSOVOD_BF16X2
                                    ? (d->ldr % 32 == 0 && ((uintptr_t)d->residual & 15) == 0)
                                : d->dtype_r == WSOVOD_BF16 ? (d->ldr % 4 == 0 && ((uintptr_t)d->residual & 7) == 0)
                                                            : (d->dtype_r == WSOVOD_F32 && d->ldr % 4 == 0 && ((uintptr_t)d->residual & 15) == 0)),
               "wsovod_gemm_f16mx: residual rows must be vector-aligned");
  WS_CHECK_ARG(!d->residual || d->dtype_r != WSOVOD_F16MX || d->N % 16 == 0, "wsovod_gemm_f16mx: an f16mx residual needs N a multiple of 16");

  MxArgs q;
  memset(&q, 0, sizeof(q));
  GemmArgs& a = q.g;
  fill_gemm_args(a, *d, 2);  // counted in 2-byte slots, as the bf16x2 form
  double bytes;
  if (d->conv) {
    const wsovod_conv_geom& g = d->geom;
    WS_CHECK_ARG(!a_scale, "wsovod_gemm_f16mx(conv): the input map is a unit-scale f16mx tensor (a_scale = NULL)");
    WS_CHECK_ARG(g.Cin > 0 && g.Cin % 32 == 0 && !g.pool, "wsovod_gemm_f16mx(conv): Cin=%d must be a multiple of 32 (no fused pool)", g.Cin);
    if (int rc = check_and_fill_conv(a, *d, 2, 2, 32, /*border_in_limit=*/true, "wsovod_gemm_f16mx")) return rc;
    if (br)
      if (int rc = check_branch_limit(a, *br, "wsovod_gemm_f16mx_conv_branches")) return rc;
    bytes = ((double)g.n_img * g.H * g.W * g.Cin + (double)d->N * d->K + (d->A2 ? (double)d->M * d->Cin2 : 0.0)) * 4.0;
  } else {
    WS_CHECK_ARG(a_segments == 1 || a_scale, "wsovod_gemm_f16mx: scale segments without a scale array");
    WS_CHECK_ARG(d->lda % 4 == 0 && d->lda >= d->K && 320ll * d->lda * 4 < (1ll << 31),
                 "wsovod_gemm_f16mx: lda=%lld: f16mx rows of at least K values, a tile of rows below 2 GiB", d->lda);
    bytes = ((double)d->M + d->N) * d->K * 4.0;
  }
  bytes += (double)d->M * d->N * ((d->dtype_c == WSOVOD_BF16 ? 2 : 4) + (c_bf16 ? 2 : 0) + (d->residual ? (d->dtype_r == WSOVOD_BF16 ? 2 : 4) : 0));
  const int nbr = br ? br->n_branch : 1;
  if (br) bytes = bytes * nbr - (double)(nbr - 1) * d->N * d->K * 4.0;  // (the weight is read once)
  a.tiles_m = (d->M + 255) / 256 * nbr;
  a.tiles_n = (d->N + 255) / 256;
  a.group_m = tile_group_height(a.tiles_m, a.tiles_n, 4);
  q.sa = d->conv ? nullptr : a_scale;
  q.sb = b_scale;
  q.nseg_a = a_scale ? a_segments : 1;
  q.nseg_b = b_segments;
  q.c_bf16 = c_bf16;
  q.ld_cb = ld_c_bf16;
#if defined(MX_STAMPS)
  if (const char* e = getenv("WSOVOD_MX_DEBUG_PTR")) q.dbg = (float*)strtoull(e, nullptr, 16);
#endif
  static int slot_g = wsovod::prof_slot("gemm_nt_f16mx_256x256_8ph"), slot_c = wsovod::prof_slot("conv_igemm_f16mx_256x256_8ph");
  static bool attr_set = false;
  constexpr int lds_bytes = (3 * 256 + 2 * 256) * 128;  // 160 KiB: the whole CU
  if (!attr_set) {
#define MX_OPT_IN(C, E) WS_OPT_IN_LDS((gemm256_mx_kernel<C, E>), lds_bytes, "wsovod_gemm_f16mx: LDS opt-in")
    MX_OPT_IN(false, 0); MX_OPT_IN(false, 1); MX_OPT_IN(false, 4);
    MX_OPT_IN(true, 0); MX_OPT_IN(true, 1); MX_OPT_IN(true, 2); MX_OPT_IN(true, 3);
#undef MX_OPT_IN
#define MX_OPT_IN_T(E) WS_OPT_IN_LDS((gemm256_mx_kernel<true, E, true>), lds_bytes, "wsovod_gemm_f16mx: LDS opt-in")
    MX_OPT_IN_T(0); MX_OPT_IN_T(1); MX_OPT_IN_T(2); MX_OPT_IN_T(3);
#undef MX_OPT_IN_T
    WS_OPT_IN_LDS((gemm256_mx_br_kernel<true, 0>), lds_bytes, "wsovod_gemm_f16mx_conv_branches: LDS opt-in");
    WS_OPT_IN_LDS((gemm256_mx_br_kernel<true, 1>), lds_bytes, "wsovod_gemm_f16mx_conv_branches: LDS opt-in");
#define MX_OPT_IN_X(E) WS_OPT_IN_LDS((gemm256_mx_brx_kernel<true, E>), lds_bytes, "wsovod_gemm_f16mx_conv_branches_ex: LDS opt-in")
    MX_OPT_IN_X(0); MX_OPT_IN_X(1); MX_OPT_IN_X(2); MX_OPT_IN_X(3);
#undef MX_OPT_IN_X
    attr_set = true;
  }
  hipStream_t s = (hipStream_t)stream;
  // ---- the last, partly filled round of tiles.  One 256 x 256 tile per CU and launch round: a launch of T tiles costs
  // ceil(T / CUs) tile times -- res5 of 32 images is 1876 tiles = 7.33 rounds.  The rows of the last round go to a SECOND
  // launch of the same kernel whose grid is S copies of those tiles, copy z reducing a slice of the K-steps into an fp32
  // workspace, and a finalize pass adds the slices and applies the epilogue: S is chosen so that the copies fill whole rounds
  // again (res5: 84 tiles x 3 = 252).  Measured (tools/mx_conv_ab.py, 32 images): res5 1.833 -> 1.780 ms per conv; a last
  // round that is more than half full (res4: 170 tiles) is left alone -- its slices' workspace traffic and shorter K loops cost
  // more than the idle CUs, which the chip gives back as clock under its power limit (0.509 -> 0.560 ms with 170 x 3).
  int n_cu = wsovod::cu_count();
  // (WSOVOD_MX_TAIL_CUS=n: the round arithmetic below as on a chip of n CUs -- tests reach the K-slices at a few tiles)
  if (const char* e = getenv("WSOVOD_MX_TAIL_CUS"))
    if (atoi(e) > 0) n_cu = atoi(e);
  const int ntiles = a.tiles_m * a.tiles_n, nk_all = a.K / 64;
  int tail_mt = 0, S = 1;
  {
    // (the branch-batched form keeps ONE launch: its last round is the branches' last tiles, whose rows are not contiguous)
    // (WSOVOD_MX_TAIL=0: one launch; A/B runs)
    const bool on = !br && !wsovod::env_off("WSOVOD_MX_TAIL") && q.nseg_a == 1 && q.nseg_b == 1 && n_cu % a.tiles_n == 0 && nk_all >= 24;
    const int rem = ntiles % n_cu;
    if (on && ntiles > n_cu && rem != 0 && rem % a.tiles_n == 0 && 2 * rem <= n_cu) {
      double best = 1.0 + 0.02;
      for (int c = 2; c <= 8 && nk_all / c >= 12; ++c) {
        const double cost = (double)((rem * c + n_cu - 1) / n_cu) / c + 0.02 * c;
        if (cost < best - 1e-9) best = cost, S = c;
      }
      if (S > 1) tail_mt = rem / a.tiles_n;
    }
  }
  if (tail_mt > 0) {
    // doubling workspace (wsovod::Scratch); where it would have to grow under stream capture, or cannot be allocated, the
    // conv silently runs as the single launch -- another summation order for the last round's rows than outside the capture
    static wsovod::Scratch ws(wsovod::ScratchGrowth::doubling());
    const int m_base = (a.tiles_m - tail_mt) * 256;
    const long long ldp = ((long long)d->N + 3) / 4 * 4;
    wsovod::ScratchStatus st;
    a.partial = (float*)ws.reserve((size_t)S * (d->M - m_base) * ldp * sizeof(float), s, &st);
    if (a.partial) a.partial_ld = ldp;
    else tail_mt = 0;
  }
  static int slot_b = wsovod::prof_slot("conv_igemm_f16mx_256x256_8ph_branches");
  static int slot_bx = wsovod::prof_slot("conv_igemm_f16mx_256x256_8ph_branches_ex");
  wsovod::ProfScope prof(br ? (ex ? slot_bx : slot_b) : d->conv ? slot_c : slot_g, s, 2.0 * d->M * nbr * (double)d->N * d->K, bytes);
  if (br && ex) {
    MxBrExArgs qb;
    memset(&qb, 0, sizeof(qb));
    static_cast<MxArgs&>(qb) = q;
    qb.tiles_per_branch = (d->M + 255) / 256;
    for (int b = 0; b < 4; ++b) {
      qb.dil[b] = br->dil[b < nbr ? b : 0];
      qb.pad[b] = br->pad[b < nbr ? b : 0];
    }
    qb.a_branch_bytes = br->shared_input ? 0 : a.a_bytes;
    qb.c_branch_bytes = (long long)d->M * d->ldc * 4;
    qb.r_branch_bytes = (!d->residual || *ex) ? 0 : (long long)d->M * d->ldr * (d->dtype_r == WSOVOD_BF16 ? 2 : 4);
    // (EPI exactly as the single-dilation conv entry chooses it below: the same build of the epilogue, the same bits)
    const bool mxr = d->residual && d->dtype_r == WSOVOD_F16MX;
    const int epi = d->N % 64 != 0 ? 0 : (d->dtype_c == WSOVOD_F16MX && !d->residual) ? 1 : (d->dtype_c == WSOVOD_F16MX && mxr) ? 2
                    : (d->dtype_c == WSOVOD_F32 && mxr) ? 3 : 0;
#define MX_LAUNCH_X(E) hipLaunchKernelGGL((gemm256_mx_brx_kernel<true, E>), dim3(ntiles), dim3(512), lds_bytes, s, qb)
    if (epi == 1) MX_LAUNCH_X(1);
    else if (epi == 2) MX_LAUNCH_X(2);
    else if (epi == 3) MX_LAUNCH_X(3);
    else MX_LAUNCH_X(0);
#undef MX_LAUNCH_X
    WS_CHECK_LAUNCH("wsovod_gemm_f16mx_conv_branches_ex");
    return WSOVOD_OK;
  }
  if (br) {
    MxBrArgs qb;
    memset(&qb, 0, sizeof(qb));
    static_cast<MxArgs&>(qb) = q;
    qb.tiles_per_branch = (d->M + 255) / 256;
    for (int b = 0; b < 4; ++b) {
      qb.dil[b] = br->dil[b < nbr ? b : 0];
      qb.pad[b] = br->pad[b < nbr ? b : 0];
    }
    qb.a_branch_bytes = br->shared_input ? 0 : a.a_bytes;
    qb.c_branch_bytes = (long long)d->M * d->ldc * 4;
    // (EPI as below: 1 = f16mx out of whole 64-column blocks, else the general epilogue)
    if (d->N % 64 == 0 && d->dtype_c == WSOVOD_F16MX)
      hipLaunchKernelGGL((gemm256_mx_br_kernel<true, 1>), dim3(ntiles), dim3(512), lds_bytes, s, qb);
    else
      hipLaunchKernelGGL((gemm256_mx_br_kernel<true, 0>), dim3(ntiles), dim3(512), lds_bytes, s, qb);
    WS_CHECK_LAUNCH("wsovod_gemm_f16mx_conv_branches");
    return WSOVOD_OK;
  }
  auto launch = [&](const MxArgs& qq, int grid) {
    // the epilogue form (the kernel's EPI): the hot combinations have their own builds
    const bool mxr = d->residual && d->dtype_r == WSOVOD_F16MX;
    const int epi = (d->N % 64 != 0 || qq.g.ksplit > 1 || (d->conv && (d->dropout_p > 0.f || c_bf16))) ? 0
                    : (d->dtype_c == WSOVOD_F16MX && !d->residual) ? 1
                    : (d->dtype_c == WSOVOD_F16MX && mxr && d->conv) ? 2
                    : (d->dtype_c == WSOVOD_F32 && mxr && d->conv) ? 3
                    : (d->dtype_c == WSOVOD_BF16X2 && !d->residual && !d->conv) ? 4 : 0;
#define MX_LAUNCH(C, E) hipLaunchKernelGGL((gemm256_mx_kernel<C, E>), dim3(grid), dim3(512), lds_bytes, s, qq)
#define MX_LAUNCH_T(E) hipLaunchKernelGGL((gemm256_mx_kernel<true, E, true>), dim3(grid), dim3(512), lds_bytes, s, qq)
    // the conv's tap state as running offsets (the kernel's TAPTAB) unless WSOVOD_MX_TAPTAB=0 (the (r, q, c0) form: A/B runs,
    // tests/test_gpu_mx_conv_taptable.py; kept for one release) or a border tap's offset | 2^31 + its scalar offset could
    // reach 2^32 (maps next to the 2 GiB limit)
    const long long span = qq.g.a_bytes + 2ll * ((long long)(qq.g.KH - 1) * qq.g.dil * qq.g.W + (long long)(qq.g.KW - 1) * qq.g.dil + 1) * qq.g.Cin * 2 + 128;
    if (d->conv && !wsovod::env_off("WSOVOD_MX_TAPTAB") && span < (1ll << 31)) {
      if (epi == 1) MX_LAUNCH_T(1);
      else if (epi == 2) MX_LAUNCH_T(2);
      else if (epi == 3) MX_LAUNCH_T(3);
      else MX_LAUNCH_T(0);
    } else if (d->conv) {
      if (epi == 1) MX_LAUNCH(true, 1);
      else if (epi == 2) MX_LAUNCH(true, 2);
      else if (epi == 3) MX_LAUNCH(true, 3);
      else MX_LAUNCH(true, 0);
    } else {
      if (epi == 1) MX_LAUNCH(false, 1);
      else if (epi == 4) MX_LAUNCH(false, 4);
      else MX_LAUNCH(false, 0);
    }
#undef MX_LAUNCH
#undef MX_LAUNCH_T
  };
  if (tail_mt == 0) {
    launch(q, ntiles);
  } else {
    MxArgs qm = q;  // whole rounds: rows [0, m_base)
    const int m_base = (a.tiles_m - tail_mt) * 256;
    qm.g.M = m_base;
    qm.g.tiles_m = a.tiles_m - tail_mt;
    qm.g.partial = nullptr;
    launch(qm, qm.g.tiles_m * a.tiles_n);
    MxArgs qt = q;  // the last round's rows [m_base, M), S slices of K
    qt.g.m_base = m_base;
    qt.g.tiles_m = tail_mt;
    qt.g.ksplit = S;
    qt.g.slice_steps = (nk_all + S - 1) / S;
    qt.g.group_m = tile_group_height(tail_mt, a.tiles_n, 4);
    launch(qt, tail_mt * a.tiles_n * S);
    const long long quads = (long long)(d->M - m_base) * (d->N / 4);
    hipLaunchKernelGGL(mx_splitk_finalize_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, qt);
  }
  WS_CHECK_LAUNCH("wsovod_gemm_f16mx");
  return WSOVOD_OK;
}

extern "C" int wsovod_gemm_f16mx(const wsovod_gemm_desc* d, const unsigned char* a_scale, int a_segments,
                                 const unsigned char* b_scale, int b_segments, void* c_bf16, long long ld_c_bf16,
                                 wsovod_stream_t stream) {
  return gemm_f16mx_impl(d, a_scale, a_segments, b_scale, b_segments, c_bf16, ld_c_bf16, nullptr, stream);
}

extern "C" int wsovod_gemm_f16mx_conv_branches(const wsovod_gemm_desc* d, const wsovod_conv_branches* br,
                                               const unsigned char* b_scale, int b_segments, wsovod_stream_t stream) {
  WS_CHECK_ARG(br, "wsovod_gemm_f16mx_conv_branches: null branch descriptor");
  return gemm_f16mx_impl(d, nullptr, 1, b_scale, b_segments, nullptr, 0, br, stream);
}

extern "C" int wsovod_gemm_f16mx_conv_branches_ex(const wsovod_gemm_desc* d, const wsovod_conv_branches* br, int residual_shared,
                                                  const unsigned char* b_scale, int b_segments, wsovod_stream_t stream) {
  WS_CHECK_ARG(br, "wsovod_gemm_f16mx_conv_branches_ex: null branch descriptor");
  return gemm_f16mx_impl(d, nullptr, 1, b_scale, b_segments, nullptr, 0, br, stream, &residual_shared);
}
