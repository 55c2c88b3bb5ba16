// pass_render.h — the depth-map evaluation on the device (dpe_cloud_render_view and dpe_depth_score of
// include/dpe_mvs.h, which states the contract).  The arithmetic is depth_eval.h's, which the host loops
// (host/depth_eval.cpp) share.
//
//   k_render_clear   one thread per pixel: the z-buffer's word becomes +inf's bits, "no point yet"
//   k_render_splat   one thread per scan point: its centre pixel and the bits of its depth, then an integer
//                    atomicMin on every pixel of its splat inside the image.  Positive finite floats order as their
//                    bits, so the word ends as the bits of the minimum depth whatever the schedule.  A plain load
//                    first skips the atomic where the word is already as small: the words only ever fall, so a
//                    stale value can make a thread try an atomic it did not need, never skip one it did
//   k_render_finish  one thread per pixel: +inf's bits become 0.0f; the buffer is then the map, f32 [h][w]
//   k_depth_score    block = 256 consecutive pixels: every thread forms its pixel's three terms (+0.0 unless both
//                    depths are usable), the block sums them by the butterfly of tree_sum.h, and k_tree_reduce<3>
//                    takes the block results from there; the counters go by ballot and
//                    popcount into one LDS slot per wave and counter, then one integer atomic per block and counter
//
// No float atomics, no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include "depth_eval.h"
#include "tree_sum.h"

namespace dpe {

constexpr int kRenderBlock = kTreeBlock;
constexpr int kDepthCounters = 3 + DPE_DEPTH_MAX_TAU;   // n_gt, n_est, n_both, within[16]

struct DepthTaus {
  float tau[DPE_DEPTH_MAX_TAU];
  int n, mode;
};

__global__ void __launch_bounds__(kRenderBlock) k_render_clear(uint32_t* __restrict__ zb, size_t npx) {
  const size_t i = (size_t)blockIdx.x * kRenderBlock + threadIdx.x;
  if (i < npx) zb[i] = kDepthEmpty;
}

__global__ void __launch_bounds__(kRenderBlock) k_render_splat(const float* __restrict__ pts, int n, DpeCamera cam, int s,
                                                               uint32_t* zb) {
  const size_t i = (size_t)blockIdx.x * kRenderBlock + threadIdx.x;
  if (i >= (size_t)n) return;
  int cx, cy;
  uint32_t z;
  if (!depth_point(cam, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], cx, cy, z)) return;
  const int w = cam.width, h = cam.height;
  const int x0 = cx - s < 0 ? 0 : cx - s, x1 = cx + s > w - 1 ? w - 1 : cx + s;
  const int y0 = cy - s < 0 ? 0 : cy - s, y1 = cy + s > h - 1 ? h - 1 : cy + s;
  for (int y = y0; y <= y1; ++y) {
    uint32_t* row = zb + (size_t)y * (size_t)w;
    for (int x = x0; x <= x1; ++x)
      if (z < __atomic_load_n(row + x, __ATOMIC_RELAXED)) atomicMin(row + x, z);
  }
}

__global__ void __launch_bounds__(kRenderBlock) k_render_finish(uint32_t* __restrict__ zb, size_t npx) {
  const size_t i = (size_t)blockIdx.x * kRenderBlock + threadIdx.x;
  if (i < npx && zb[i] == kDepthEmpty) zb[i] = 0u;
}

// part: 3 doubles per block; counts: kDepthCounters words; err: the error map or null
__global__ void __launch_bounds__(kRenderBlock) k_depth_score(const float* __restrict__ est, const float* __restrict__ gt,
                                                              size_t npx, DepthTaus T, double* __restrict__ part,
                                                              unsigned long long* __restrict__ counts,
                                                              float* __restrict__ err) {
  __shared__ int wc[kRenderBlock / 64][kDepthCounters];
  const size_t i = (size_t)blockIdx.x * kRenderBlock + threadIdx.x;
  const bool in = i < npx;
  const float g = in ? gt[i] : 0.0f;
  DepthPixel p = depth_pixel(in ? est[i] : 0.0f, g);   // past the end: neither depth is usable
  double t[kDepthTerms];
  depth_terms(p, t);
  if (in && err) err[i] = depth_error_code(p);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c_gt = __popcll(__ballot(p.gt_ok)), c_est = __popcll(__ballot(p.est_ok)), c_both = __popcll(__ballot(p.both));
  if (lane == 0) { wc[wave][0] = c_gt; wc[wave][1] = c_est; wc[wave][2] = c_both; }
  for (int k = 0; k < T.n; ++k) {
    const int c = __popcll(__ballot(depth_hit(p, g, T.tau[k], T.mode)));
    if (lane == 0) wc[wave][3 + k] = c;
  }
  block_tree_sum<kDepthTerms>(t, part + (size_t)blockIdx.x * kDepthTerms);   // its barrier also publishes wc
  if ((int)threadIdx.x < 3 + T.n) {
    const int k = threadIdx.x;
    const int all = wc[0][k] + wc[1][k] + wc[2][k] + wc[3][k];
    if (all > 0) atomicAdd(counts + k, (unsigned long long)all);
  }
}

}  // namespace dpe
