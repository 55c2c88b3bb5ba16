// tap_launch.hip — launches of the strong sweep, DepthToWeak and LocalRefine on the 8-bit /
// quarter-integer texel layouts, their own translation unit; the f32-texel instantiations are in
// tap_f32.hip.
//
// A scheduler is chosen per compilation.  Rounds 2-4 compiled these kernels with LLVM's
// occupancy-first iterative scheduler (-mllvm -amdgpu-sched-strategy=iterative-maxocc): the
// default one then hoisted the unrolled 36-tap loop's gathers past 128 VGPRs and spilled.  Since
// round 5's tap reciprocal (no Newton step) and rolled slow-patch loop the default scheduler fits
// them in 113-124 VGPRs with no scratch, and is faster: strong 26.56 -> 25.99 ms, DepthToWeak
// 21.81 -> 20.94 ms, wall 67.63 -> 65.73 ms (profiles/r05ad_ab_tapsched.log, bit-identical).  The
// f32 instantiations still spill under the default (164-244 B/lane) and keep the iterative
// scheduler in tap_f32.hip.  The weak sweep stays in dpe_mvs.hip with the default.
// Of the library's units (the Makefile's table) only this one, tap_f32.hip and dpe_mvs.hip compile
// pass kernels; each of the three has its own copy of the DPE_DIAG counters and its own readers
// (DPE_DBG_READER, tap_launch.h), and a launch that needs more than 64 KB of LDS goes through
// allow_large_lds (tap_launch.h).
#define DPE_TAP_TU 1
#include "tap_launch.h"
#include "pass_refine.h"
#include "pass_sweep.h"

namespace dpe {

void launch_strong(bool edge, int cls, unsigned grid, size_t lds, hipStream_t s, const PassConst* dpc,
                   const DevBufs& B, int it, const int* list, const int* count) {
  constexpr int T = 64 * kBwStrong;
  if (cls == IMG_F32) { launch_strong_f32(edge, grid, lds, s, dpc, B, it, list, count); return; }
  if (edge) {
    allow_large_lds<k_strong_coop<kTexStrong, true>>(lds);
    k_strong_coop<kTexStrong, true><<<grid, T, lds, s>>>(dpc, B, it, list, count);
  } else {
    allow_large_lds<k_strong_coop<kTexStrong, false>>(lds);
    k_strong_coop<kTexStrong, false><<<grid, T, lds, s>>>(dpc, B, it, list, count);
  }
}

void launch_depth_to_weak(int cls, bool wide, long L, hipStream_t s, const PassConst* dpc, const DevBufs& B) {
  const unsigned g = (unsigned)((L + kBwD2W - 1) / kBwD2W);
  if (cls == IMG_F32) { launch_depth_to_weak_f32(g, s, dpc, B); return; }
  static_assert(kTexD2W == TEX_F16 && kTexLR == TEX_F16 && kTexStrong != TEX_F16, "the wide twins below");
  if (wide) k_depth_to_weak<TEX_F16W, true><<<g, 64 * kBwD2W, 0, s>>>(dpc, B);
  else k_depth_to_weak<kTexD2W, true><<<g, 64 * kBwD2W, 0, s>>>(dpc, B);
}

void launch_local_refine(int cls, bool wide, long L, int W, int H, int nv, hipStream_t s, const PassConst* dpc, const DevBufs& B) {
  // with the fused DepthToWeak only its border pixels are left
  const int border = 1;
  L = border_count(W, H);
  const unsigned g = (unsigned)((L + kBwLR * kLrPix - 1) / (kBwLR * kLrPix));
  if (g == 0) return;
  const size_t lds = (size_t)kBwLR * kLrPix * 12 * nv * 2 * sizeof(float);
  if (cls == IMG_F32) { launch_local_refine_f32(g, lds, border, s, dpc, B); return; }
  if (wide) {
    allow_large_lds<k_local_refine_jobs<TEX_F16W>>(lds);
    k_local_refine_jobs<TEX_F16W><<<g, 64 * kBwLR, lds, s>>>(dpc, B, border);
    return;
  }
  allow_large_lds<k_local_refine_jobs<kTexLR>>(lds);
  k_local_refine_jobs<kTexLR><<<g, 64 * kBwLR, lds, s>>>(dpc, B, border);
}

}  // namespace dpe

// this unit's own copies of the DPE_DIAG counters
#if DPE_POOL_STATS
DPE_DBG_READER(pool, tap, dpe::g_pool, 24)
DPE_DBG_READER(tail, tap, dpe::g_tail, 8)
#endif
#if DPE_LINE_STATS
DPE_DBG_READER(line, tap, dpe::g_lstat, 16)
#endif
