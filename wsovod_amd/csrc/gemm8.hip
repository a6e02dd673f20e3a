// bf16 256x256x64 GEMM / implicit-GEMM tile in the "8-phase" shape (cdna_hip_programming.md section 5, "The 256^2
// 8-phase template"), written for this library's operand layout and epilogue.
//
//   * 512 threads = 8 wavefronts as 2 (M) x 4 (N); a wavefront owns 128 x 64 of the tile = 8 x 4 MFMA tiles
//     (128 accumulator VGPRs), so a K-step reads (128 + 64) rows x 128 B of fragments per wavefront: 192 KiB per
//     workgroup against 256 KiB for 16 wavefronts of 64 x 64 -- the LDS array is no longer half as busy as the MFMA.
//   * A K-step is four PHASES, one 64 x 32 quadrant of the wavefront's output each (16 MFMAs):
//         phase 1: A rows 0-63, B cols 0-31  (12 ds_read_b128)   quadrant (lo, lo)
//         phase 2:              B cols 32-63 ( 4)                 quadrant (lo, hi)
//         phase 3: A rows 64-127             ( 8, reuse A regs)   quadrant (hi, hi)
//         phase 4: nothing to read                                quadrant (hi, lo)
//     every phase is  [fragment reads, LDS-DMA issue]  s_barrier  [16 MFMA at raised priority]  s_barrier.
//   * The two M-halves of the workgroup (wavefronts 0-3 / 4-7, one of each per SIMD) run STAGGERED by one barrier:
//     while one group is in its MFMA section the other is in its read/stage section, so the matrix pipe and the
//     LDS array are both busy all the time instead of alternating.
//   * Staging is LDS-direct (buffer_load ... lds), two K-step buffers (128 KiB), two DMA instructions per phase,
//     issued as early as the LDS rows they overwrite are free (>= 2 phases after their last read) and retired by
//     COUNTED s_waitcnt vmcnt(N) that leave the younger ones in flight -- the prefetch runs 2-5 phases ahead of its
//     use and crosses the barriers.  Every wait sits before a barrier that each reader passes before it reads
//     those rows, also the staggered group (the "one barrier more" rule of the guide).
//   * Fragment reads are inline asm: hipcc would otherwise put s_waitcnt vmcnt(0) in front of every ds_read it can
//     see while an LDS-DMA is outstanding and drain the prefetch at once.
// Same XOR swizzle (chunk ^ ((row >> 1) & 7), applied to the DMA source address and to the read address), XCD-aware
// grouped tile order and epilogue as gemm.hip.
#include "gemm_common.h"
#include <string.h>

namespace wsovod_gemm {

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

// X3 (bf16x2 operands, include/wsovod_hip.h): the 128-byte LDS row of a K-step holds the hi halves of 32 values in its
// chunks 0-3 and their lo halves in chunks 4-7, so the SAME two fragment reads per tile (k-half 0 / 1 of the bf16 form)
// deliver (a_hi, a_lo) and (b_hi, b_lo), and a quadrant phase issues 24 MFMAs -- bh*ah, bl*ah, bh*al -- on them instead of
// 16: staging, LDS traffic and barriers of a bf16 GEMM over 2K elements, 1.5x its MFMA work (= 3x the bf16 GEMM over K).
// PH = 2 ("merged" form): a K-step is TWO phases -- (A rows 0-63 x all 64 columns) and (A rows 64-127 x all 64 columns) --
// each [fragment reads, LDS-DMA issue, counted wait] barrier [32 (bf16) / 48 (X3) MFMAs] barrier: half the barriers and
// wait points per MFMA of the four-phase form.  Every group measured ~450 cycles per phase in which its SIMD's matrix
// pipe idles whatever the phase's MFMA count (bf16: 16 MFMAs = 256 cycles at 55 % busy; X3: 24 MFMAs = 384 cycles at
// 61 %), so doubling the MFMAs per phase raises the busy share.  DMA schedule: phase A stages B and A_lo of K-step kt+1
// (their LDS rows were last read two phases earlier) and waits for A_hi(kt); phase B stages A_hi(kt+1) and waits for the
// six instructions of phase A.  Same products in the same order as PH = 4: bit-identical results.
// LEAN (round 5, two-phase form only; K a whole number of K-steps): the half of a phase that the other group's MFMAs have
// to cover -- fragment reads + DMA issue + the counted wait -- without its address arithmetic (s_memtime stamps,
// tools/g8_phases.py: the read section of phase A took 737 ticks on a plain GEMM against 586 (bf16) / 840 (bf16x2) of MFMAs,
// and 1130 on the implicit-GEMM conv, whose tap decode / validity selects sat in front of every DMA instruction):
//  * fragment reads address four per-lane constants; the K-step buffer and the 16-row block are the instruction's
//    immediate offset (K loop unrolled by two);
//  * a DMA instruction = a per-lane CONSTANT offset (rows / columns outside the matrix: 2^31, beyond the resource's range)
//    + a scalar K offset in `soffset` (it takes part in the hardware range check on gfx950: tools/soffset_probe.hip);
//  * conv: the per-lane offsets of the NEXT K-step's tap (the pixel offset where the tap lies inside the image, 2^31
//    where it does not) are computed under the MFMAs of phase B, not in front of the DMA.
template <int OFF>
__device__ __forceinline__ void g8_read_imm(__attribute__((ext_vector_type(4))) unsigned int& dst, unsigned addr) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
#endif
}

#include "gemm8_kernel.h"
#define WSOVOD_CONV_BRANCHES 1
#include "gemm8_kernel.h"
#define WSOVOD_CONV_BRANCHES_EX 1
#include "gemm8_kernel.h"
#undef WSOVOD_CONV_BRANCHES_EX
#undef WSOVOD_CONV_BRANCHES

// split-K finalize: C[m][n] = epilogue(sum over the K slices) -- the epilogue chain of the GEMM kernels, element-wise
__global__ __launch_bounds__(256) void splitk_finalize_kernel(const GemmArgs p) {
  const int n4 = (p.N + 3) >> 2;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int rows = p.M - p.m_base;
  if (idx >= (long long)rows * n4) return;
  const int mr = (int)(idx / n4), nb = (int)(idx - (long long)mr * n4) * 4, m = p.m_base + mr;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  for (int z = 0; z < p.ksplit; ++z) {
    const float* src = p.partial + ((long long)z * rows + mr) * p.partial_ld + nb;
    if (nb + 3 < p.N) {
      const f32x4 t = *(const f32x4*)src;
      v[0] += t[0]; v[1] += t[1]; v[2] += t[2]; v[3] += t[3];
    } else {
      for (int r = 0; r < 4; ++r)
        if (nb + r < p.N) v[r] += src[r];
    }
  }
  epilogue_store4(p, m, nb, v);
}

}  // namespace

// The branch-batched bf16x2 conv: ONE launch of the lean two-phase tile over n_branch stacks of row tiles (a.M, a.a_bytes:
// one branch's).  No split-K: the single-launch summation order of the tile, per branch.
static void branch_grid(GemmBrArgs& args, const GemmArgs& a, int n_branch, const int* dil, const int* pad, bool shared_input) {
  static_cast<GemmArgs&>(args) = a;
  args.tiles_per_branch = ceil_div(a.M, 256);
  args.tiles_m = args.tiles_per_branch * n_branch;
  args.tiles_n = ceil_div(a.N, 256);
  args.group_m = tile_group_height(args.tiles_m, args.tiles_n, 4);
  args.ksplit = args.slice_steps = 0;
  args.m_base = 0;
  for (int b = 0; b < 4; ++b) {
    args.dil[b] = dil[b < n_branch ? b : 0];
    args.pad[b] = pad[b < n_branch ? b : 0];
  }
  args.a_branch_bytes = shared_input ? 0 : a.a_bytes;
  args.c_branch_bytes = (long long)a.M * a.ldc * 4;
}

int launch_gemm256_8ph_branches(const GemmArgs& a, int n_branch, const int* dil, const int* pad, bool shared_input,
                                hipStream_t s, double flops, double bytes) {
  static int slot = wsovod::prof_slot("conv_igemm_bf16x2_256x256_8ph_branches");
  static bool attr_set = false;
  constexpr int lds_bytes = 2 * (256 + 256) * 128;
  if (!attr_set) {
    WS_OPT_IN_LDS((gemm256_8ph_br_kernel<true, true, 2, true>), lds_bytes, "wsovod_gemm_conv_branches: LDS opt-in");
    attr_set = true;
  }
  GemmBrArgs args;
  memset(&args, 0, sizeof(args));
  branch_grid(args, a, n_branch, dil, pad, shared_input);
  wsovod::ProfScope prof(slot, s, flops, bytes);
  hipLaunchKernelGGL((gemm256_8ph_br_kernel<true, true, 2, true>), dim3(args.tiles_m * args.tiles_n), dim3(512), lds_bytes, s, args);
  WS_CHECK_LAUNCH("wsovod_gemm_conv_branches(256x256 8-phase)");
  return WSOVOD_OK;
}

// wsovod_gemm_conv_branches_ex: the same grid on gemm256_8ph_brx_kernel, whose prologue also moves the residual pointer to
// the tile's branch (shared_residual: every branch adds the SAME (M, N) rows, block 0 of an MRRP residual stage)
int launch_gemm256_8ph_branches_ex(const GemmArgs& a, int n_branch, const int* dil, const int* pad, bool shared_input,
                                   bool shared_residual, hipStream_t s, double flops, double bytes) {
  static int slot = wsovod::prof_slot("conv_igemm_bf16x2_256x256_8ph_branches_ex");
  static bool attr_set = false;
  constexpr int lds_bytes = 2 * (256 + 256) * 128;
  if (!attr_set) {
    WS_OPT_IN_LDS((gemm256_8ph_brx_kernel<true, true, 2, true>), lds_bytes, "wsovod_gemm_conv_branches_ex: LDS opt-in");
    attr_set = true;
  }
  GemmBrExArgs args;
  memset(&args, 0, sizeof(args));
  branch_grid(args, a, n_branch, dil, pad, shared_input);
  args.r_branch_bytes = (!a.residual || shared_residual) ? 0 : (long long)a.M * a.ldr * (a.dtype_r == WSOVOD_BF16 ? 2 : 4);
  wsovod::ProfScope prof(slot, s, flops, bytes);
  hipLaunchKernelGGL((gemm256_8ph_brx_kernel<true, true, 2, true>), dim3(args.tiles_m * args.tiles_n), dim3(512), lds_bytes, s, args);
  WS_CHECK_LAUNCH("wsovod_gemm_conv_branches_ex(256x256 8-phase)");
  return WSOVOD_OK;
}

int launch_gemm256_8ph(const GemmArgs& a, bool conv, hipStream_t s, double flops, double bytes, bool allow_split, bool x3,
                       bool merged) {
  allow_split = allow_split || a.ksplit == -1;  // -1: the dispatcher chose this tile itself (no tile_hint)
  static int slot_g = wsovod::prof_slot("gemm_nt_bf16_256x256_8ph");
  static int slot_c = wsovod::prof_slot("conv_igemm_bf16_256x256_8ph");
  static int slot_g3 = wsovod::prof_slot("gemm_nt_bf16x2_256x256_8ph");
  static int slot_c3 = wsovod::prof_slot("conv_igemm_bf16x2_256x256_8ph");
  static bool attr_set = false;
  constexpr int lds_bytes = 2 * (256 + 256) * 128;
  if (!attr_set) {
#define G8_OPT_IN(...) WS_OPT_IN_LDS((gemm256_8ph_kernel<__VA_ARGS__>), lds_bytes, "wsovod_gemm_nt (8-phase tile): LDS opt-in")
    G8_OPT_IN(false); G8_OPT_IN(true); G8_OPT_IN(false, true); G8_OPT_IN(true, true);
    G8_OPT_IN(false, false, 2); G8_OPT_IN(true, false, 2); G8_OPT_IN(false, true, 2); G8_OPT_IN(true, true, 2);
    G8_OPT_IN(false, false, 2, true); G8_OPT_IN(true, false, 2, true); G8_OPT_IN(false, true, 2, true); G8_OPT_IN(true, true, 2, true);
#undef G8_OPT_IN
    attr_set = true;
  }
  GemmArgs args = a;
#if defined(G8_STAMPS)
  if (const char* dp = getenv("WSOVOD_G8_DEBUG_PTR")) args.partial = (float*)strtoull(dp, nullptr, 16);
#endif
  args.tiles_m = ceil_div(a.M - a.m_base, 256);
  args.tiles_n = ceil_div(a.N, 256);
  args.group_m = tile_group_height(args.tiles_m, args.tiles_n, 4);
  // Split-K for contractions with few output tiles and a long K (the FC layers at 1-4 images per step: fc1 forward is
  // 2 x 16 tiles of K = 25088): `ksplit` copies of the grid fill the chip, each reducing a slice of K into a workspace,
  // and a finalize kernel adds the slices and applies the epilogue.  The 256x256 tile keeps the operand traffic through
  // L2 low (a 64x64 tiling of the same GEMM re-reads the operands 8x / 64x and is L2-bound at ~1 TB/s of HBM).
  args.ksplit = args.slice_steps = 0;
  const int ntiles = args.tiles_m * args.tiles_n, nk = ceil_div(a.K, 64);
  int grid = ntiles;
  // (round 5: also the implicit-GEMM convs at 1 - 4 images per step -- res5 of ONE 800x600 image is 30 x 2 tiles --
  // where the alternative was a 128x128 / 64x64 grid at 0.12 - 0.25 of peak)
  if (allow_split && ntiles <= 128 && nk >= 32) {
    int S = std::min(std::min(8, 256 / ntiles), nk / 16);
    const int forced = wsovod::env_int("WSOVOD_SPLITK_S", INT_MIN);  // (experiments)
    if (forced != INT_MIN) S = std::max(1, std::min(forced, nk / 4));
    if (S >= 2) {
      // Doubling workspace (wsovod::Scratch): the largest possible request is 8 slices x 128 tiles = 268 MB.  Growing under
      // stream capture is refused (the conv forms make `need` shape-dependent).
      static wsovod::Scratch ws(wsovod::ScratchGrowth::doubling());
      const long long ldp = ((long long)a.N + 3) / 4 * 4;
      const size_t need = (size_t)S * (a.M - a.m_base) * ldp * sizeof(float);
      wsovod::ScratchStatus st;
      float* block = (float*)ws.reserve(need, s, &st);
      if (st == wsovod::ScratchStatus::would_grow_under_capture) {
        wsovod::set_error("wsovod_gemm_nt: the split-K workspace would have to grow under stream capture; run the "
                          "shape once outside the capture first");
        return WSOVOD_ERR_UNSUPPORTED;
      }
      if (!block) {
        wsovod::set_error("wsovod_gemm_nt: cannot allocate the split-K workspace");
        return WSOVOD_ERR_HIP;
      }
      args.ksplit = S;
      args.slice_steps = ceil_div(nk, S);
      args.partial = block;
      args.partial_ld = ldp;
      grid = ntiles * S;
    }
  }
  static int slot_fin = wsovod::prof_slot("splitk_finalize");
  {
  wsovod::ProfScope prof(x3 ? (conv ? slot_c3 : slot_g3) : (conv ? slot_c : slot_g), s, flops, bytes);
#define WS_L8(C, X, P) hipLaunchKernelGGL((gemm256_8ph_kernel<C, X, P>), dim3(grid), dim3(512), lds_bytes, s, args)
#define WS_L8L(C, X) hipLaunchKernelGGL((gemm256_8ph_kernel<C, X, 2, true>), dim3(grid), dim3(512), lds_bytes, s, args)
  // the lean two-phase form: whole K-steps only (no K tail select in front of its DMA instructions)
  const bool lean = merged && a.K % 64 == 0 && !wsovod::env_off("WSOVOD_G8_LEAN") &&
                    (!conv || (a.Cin % 64 == 0 && (!a.A2 || a.Cin2 % 64 == 0) &&
                               a.a_bytes + (long long)(a.pad * a.W + a.pad) * a.Cin * 2 < (1ll << 31)));
  if (a.a_plane && !(lean && x3 && !conv)) {
    wsovod::set_error("wsovod_gemm_nt: a planar bf16x2 A operand is served by the lean two-phase tile only (plain GEMM, "
                      "K a multiple of 32 values)");
    return WSOVOD_ERR_UNSUPPORTED;
  }
  if (lean) {
    if (x3 && conv) WS_L8L(true, true);
    else if (x3) WS_L8L(false, true);
    else if (conv) WS_L8L(true, false);
    else WS_L8L(false, false);
  } else if (merged) {
    if (x3 && conv) WS_L8(true, true, 2);
    else if (x3) WS_L8(false, true, 2);
    else if (conv) WS_L8(true, false, 2);
    else WS_L8(false, false, 2);
  } else {
    if (x3 && conv) WS_L8(true, true, 4);
    else if (x3) WS_L8(false, true, 4);
    else if (conv) WS_L8(true, false, 4);
    else WS_L8(false, false, 4);
  }
#undef WS_L8
#undef WS_L8L
  }
  if (args.ksplit > 1) {
    const long long quads = (long long)(a.M - a.m_base) * ((a.N + 3) / 4);
    wsovod::ProfScope prof(slot_fin, s, 0.0, (double)quads * 16.0 * (args.ksplit + 1));
    hipLaunchKernelGGL(splitk_finalize_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, args);
  }
  WS_CHECK_LAUNCH("wsovod_gemm_nt(256x256 8-phase)");
  return WSOVOD_OK;
}

}  // namespace wsovod_gemm
