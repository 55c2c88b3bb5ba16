// tap_launch.h — source-image layout per kernel and the launchers of the tap kernels compiled in
// their own translation units (tap_launch.hip; the f32-texel instantiations in tap_f32.hip), and what
// the units that compile pass kernels share on the host side: allow_large_lds and DPE_DBG_READER.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include "pass_common.h"

// source-image layout of each kernel for 8-bit grey-level images (pass_common.h TEX_*): TEX_F16
// issues fewer VALU ops per tap, TEX_U8 touches half the bytes (better for scattered gathers),
// TEX_P16 is in between (half the bytes, 2 more ops per tap than TEX_F16, one unaligned 8-B load).
// A/B on the bench pass (two runs): P16 strong -0.85 / -0.32 ms; DepthToWeak -0.9 / +0.9 (noise),
// LocalRefine +0.2 / -0.2, weak +3 (the 8-B unaligned gathers of its scattered patches cost more)
namespace dpe {
// Grey-level class of a pass's images (dpe_pm_stage): which texel layouts hold them exactly
enum ImgClass { IMG_F32 = 0, IMG_Q = 1, IMG_U8 = 2 };   // any / multiples of 1/4 in [0, 255] / integers
constexpr int kTexInit = TEX_F16, kTexStrong = TEX_P16, kTexWeak = TEX_U8;
constexpr int kTexD2W = TEX_F16, kTexLR = TEX_F16;

// Launchers (tap_launch.hip).  cls: ImgClass of the staged images (IMG_U8 / IMG_Q: the half-precision
// layouts are staged; IMG_F32: the f32 quad image only).  wide: PassConst::tex_wide, the TEX_F16 kernels
// run as TEX_F16W (tex_addr.h).
// CheckerboardPropagationStrong + refinement, one colour's list (edge: 4 pixels x 16 lanes per wave,
// else 8 x 8); the grid and dynamic LDS are the caller's (strong_lds_per_wave).
void launch_strong(bool edge, int cls, unsigned grid, size_t lds, hipStream_t s, const PassConst* dpc,
                   const DevBufs& B, int it, const int* list, const int* count);
// DepthToWeak over the L pixels of the pass (one wave per pixel), with LocalRefine fused into its
// epilogue for interior pixels
void launch_depth_to_weak(int cls, bool wide, long L, hipStream_t s, const PassConst* dpc, const DevBufs& B);
// LocalRefine (kLrPix pixels per wave), nv source views, over the border pixels the fused
// DepthToWeak leaves
void launch_local_refine(int cls, bool wide, long L, int W, int H, int nv, hipStream_t s, const PassConst* dpc, const DevBufs& B);
// the f32-texel instantiations of the three (tap_f32.hip, occupancy-first scheduler); the grid,
// dynamic LDS and arguments are the launchers' above
void launch_strong_f32(bool edge, unsigned grid, size_t lds, hipStream_t s, const PassConst* dpc, const DevBufs& B,
                       int it, const int* list, const int* count);
void launch_depth_to_weak_f32(unsigned grid, hipStream_t s, const PassConst* dpc, const DevBufs& B);
void launch_local_refine_f32(unsigned grid, size_t lds, int border, hipStream_t s, const PassConst* dpc,
                             const DevBufs& B);

// Before a launch of `Kernel` with `bytes` of dynamic LDS: beyond the default 64 KB limit the kernel is
// allowed gfx950's 160 KB per CU, once per (kernel, device).  Keying by device is a precaution: whether
// the runtime keeps this function attribute per device has not been checked.  Threads that race here
// all set the attribute (it is idempotent); none launches before its own call has returned.
template <auto Kernel>
inline void allow_large_lds(size_t bytes) {
  if (bytes <= 65536) return;
  constexpr int kDevices = 64;
  static std::atomic<bool> done[kDevices] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kDevices) dev = -1;   // unknown: set it every time
  if (dev >= 0 && done[dev].load(std::memory_order_acquire)) return;
  (void)hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (dev >= 0) done[dev].store(true, std::memory_order_release);
}
}  // namespace dpe

// A reader of one of the DPE_DIAG counter arrays (static __device__ in pass_common.h / pass_sweep.h, so
// every unit that launches counting kernels has its own copy): dpe_dbg_<kind>_stats_<unit>(out, reset)
// copies the unit's `sym` (n values) out and optionally zeroes it.  tools/pool_stats.py and
// tools/line_stats.py sum the units' (main, tap, f32).
#define DPE_DBG_READER(kind, unit, sym, n)                                                              \
  extern "C" void dpe_dbg_##kind##_stats_##unit(unsigned long long out[n], int reset) {                 \
    static_assert(sizeof(sym) == (n) * sizeof(unsigned long long), "counter array size");               \
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(sym), sizeof(sym));                                       \
    if (reset) { unsigned long long z[n] = {}; (void)hipMemcpyToSymbol(HIP_SYMBOL(sym), z, sizeof(z)); } \
  }
