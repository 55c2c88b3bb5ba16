// pass_render.h — the renders and the score of the map evaluations on the device (dpe_cloud_render_view,
// dpe_cloud_render_view_normals, dpe_depth_score and dpe_normal_score of include/dpe_mvs.h, which states the
// contract).  The arithmetic is depth_eval.h's and normal_eval.h's, which the host loops (host/map_eval.h) share.
//
//   k_render_clear<Word>   one thread per pixel: the z-buffer's word becomes RenderWord<Word>::kEmpty, "no point yet"
//   k_render_splat<Word>   one thread per scan point: its centre pixel and its word (the bits of its depth, for the
//                          render with winners followed by its index), then an integer atomicMin on every pixel of
//                          its splat inside the image.  Positive finite floats order as their bits, so the word ends
//                          as the minimum whatever the schedule.  A plain load first skips the atomic where the word
//                          is already as small: the words only ever fall, so a stale value can make a thread try an
//                          atomic it did not need, never skip one it did
//   k_render_finish        one thread per pixel: +inf's bits become 0.0f; the buffer is then the map, f32 [h][w]
//   k_map_score<Metric>    block = 256 consecutive pixels: every thread forms its pixel's terms (+0.0 unless both
//                          values are usable), the block sums them by the butterfly of tree_sum.h, and
//                          k_tree_reduce<kTerms> takes the block results from there; the counters go by ballot and
//                          popcount into one LDS slot per wave and counter, then one integer atomic per block and
//                          counter.  A metric with a histogram (NormalMetric) finds the bin by a binary search of
//                          the edge table held in LDS and counts in kBins LDS counters per block (integer LDS
//                          atomics), flushed with one 64-bit integer atomic per non-empty bin and block
//
// No float atomics, no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include "depth_eval.h"
#include "tree_sum.h"

namespace dpe {

constexpr int kRenderBlock = kTreeBlock;

template <typename Word>
__global__ void __launch_bounds__(kRenderBlock) k_render_clear(Word* __restrict__ zb, size_t npx) {
  const size_t i = (size_t)blockIdx.x * kRenderBlock + threadIdx.x;
  if (i < npx) zb[i] = RenderWord<Word>::kEmpty;
}

template <typename Word>
__global__ void __launch_bounds__(kRenderBlock) k_render_splat(const float* __restrict__ pts, int n, DpeCamera cam, int s,
                                                               Word* zb) {
  const size_t i = (size_t)blockIdx.x * kRenderBlock + threadIdx.x;
  if (i >= (size_t)n) return;
  int cx, cy;
  uint32_t z;
  if (!depth_point(cam, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], cx, cy, z)) return;
  const Word word = RenderWord<Word>::make(z, (uint32_t)i);
  const int w = cam.width, h = cam.height;
  const int x0 = cx - s < 0 ? 0 : cx - s, x1 = cx + s > w - 1 ? w - 1 : cx + s;
  const int y0 = cy - s < 0 ? 0 : cy - s, y1 = cy + s > h - 1 ? h - 1 : cy + s;
  for (int y = y0; y <= y1; ++y) {
    Word* row = zb + (size_t)y * (size_t)w;
    for (int x = x0; x <= x1; ++x)
      if (word < __atomic_load_n(row + x, __ATOMIC_RELAXED)) atomicMin(row + x, word);
  }
}

__global__ void __launch_bounds__(kRenderBlock) k_render_finish(uint32_t* __restrict__ zb, size_t npx) {
  const size_t i = (size_t)blockIdx.x * kRenderBlock + threadIdx.x;
  if (i < npx && zb[i] == kDepthEmpty) zb[i] = 0u;
}

// the LDS of k_map_score: the counters per wave, and for a metric with a histogram the edge table and the bins
template <typename M, int Bins = M::kBins>
struct ScoreLds {
  float E[Bins];
  unsigned int hist[Bins];
  int wc[kRenderBlock / 64][3 + M::kMaxTau];
};
template <typename M>
struct ScoreLds<M, 0> {
  int wc[kRenderBlock / 64][3 + M::kMaxTau];
};

// est / gt: kChannels floats per pixel; part: kTerms doubles per block; counts: kCounters words; err: the error map
// or null; edges: the kBins bin edges (unread without bins)
template <typename M>
__global__ void __launch_bounds__(kRenderBlock) k_map_score(const float* __restrict__ est, const float* __restrict__ gt,
                                                            size_t npx, typename M::Taus T, double* __restrict__ part,
                                                            unsigned long long* __restrict__ counts, float* __restrict__ err,
                                                            const float* __restrict__ edges) {
  constexpr int C = M::kChannels;
  __shared__ ScoreLds<M> lds;
  if constexpr (M::kBins > 0) {
    if ((int)threadIdx.x < M::kBins) { lds.E[threadIdx.x] = edges[threadIdx.x]; lds.hist[threadIdx.x] = 0u; }
    __syncthreads();
  }
  const size_t i = (size_t)blockIdx.x * kRenderBlock + threadIdx.x;
  const bool in = i < npx;
  float e[C] = {}, g[C] = {};   // past the end: zeros, which no metric takes for a usable value
  if (in) {
#pragma unroll
    for (int a = 0; a < C; ++a) { e[a] = est[C * i + a]; g[a] = gt[C * i + a]; }
  }
  const typename M::Pixel p = M::pixel(e, g);
  double t[M::kTerms];
  M::terms(p, t);
  if (in && err) err[i] = M::error_code(p);
  if constexpr (M::kBins > 0) {
    if (p.both) atomicAdd(&lds.hist[M::bin(lds.E, p)], 1u);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c_gt = __popcll(__ballot(p.gt_ok)), c_est = __popcll(__ballot(p.est_ok)), c_both = __popcll(__ballot(p.both));
  if (lane == 0) { lds.wc[wave][0] = c_gt; lds.wc[wave][1] = c_est; lds.wc[wave][2] = c_both; }
  const int n_tau = T.n;   // read once: hit() takes T by reference, and the flush below would load T.n again
  for (int k = 0; k < n_tau; ++k) {
    const int c = __popcll(__ballot(M::hit(p, g, T, k)));
    if (lane == 0) lds.wc[wave][3 + k] = c;
  }
  block_tree_sum<M::kTerms>(t, part + (size_t)blockIdx.x * M::kTerms);   // its barrier also publishes wc and hist
  if ((int)threadIdx.x < 3 + n_tau) {
    const int k = threadIdx.x;
    const int all = lds.wc[0][k] + lds.wc[1][k] + lds.wc[2][k] + lds.wc[3][k];
    if (all > 0) atomicAdd(counts + k, (unsigned long long)all);
  }
  if constexpr (M::kBins > 0) {
    if ((int)threadIdx.x < M::kBins) {
      const unsigned int v = lds.hist[threadIdx.x];
      if (v > 0u) atomicAdd(counts + 3 + M::kMaxTau + threadIdx.x, (unsigned long long)v);
    }
  }
}

}  // namespace dpe
