// pass_normals.h — the normal-map evaluation on the device (dpe_cloud_normals, dpe_cloud_render_view_normals and
// dpe_normal_score of include/dpe_mvs.h, which states the contract).  The arithmetic is normal_eval.h's, which the
// host loops (host/normal_eval.cpp) share.
//
//   k_cloud_normal        one thread per finite point in BUCKET order over the grid that k_cloud_count / _scan / _fill
//                         built from the same cloud: cloud_walk's 27 cells, but the ten int64 sums instead of a minimum,
//                         then the 3 x 3 solve in the same thread; written back by original index.  NO POINT TWICE: a
//                         cell whose bucket an earlier cell of the 27 already gave is skipped (normal_eval.h says why
//                         that counts every neighbour exactly once)
//   k_render_clear64      one thread per pixel: the z-buffer's 64-bit word becomes (+inf's bits, index -1)
//   k_render_splat_idx    k_render_splat with the word bits(z) << 32 | point index: a 64-bit integer atomicMin behind
//                         the same plain-load skip; the word ends as the lexicographic minimum of (bits(z), index)
//   k_render_finish_idx   one thread per pixel: the word split into the f32 map and the i32 winner, -1 where empty
//   k_render_normals      one thread per pixel: the winner's normal turned towards the camera, zeros without one
//   k_normal_score        block = 256 consecutive pixels: the two terms through block_tree_sum<2> (k_tree_reduce<2>
//                         goes on from there), the counters by ballot and popcount as in k_depth_score, the bin by a
//                         binary search of the edge table held in LDS, the histogram in 180 LDS counters per block
//                         (integer LDS atomics) flushed with one 64-bit integer atomic per non-empty bin and block
//
// No float atomics, no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include "normal_eval.h"
#include "tree_sum.h"

namespace dpe {

constexpr int kNormalBlock = kTreeBlock;
constexpr int kNormalCounters = 3 + DPE_NORMAL_MAX_TAU + DPE_NORMAL_BINS;   // n_gt, n_est, n_both, within[16], hist[180]

struct NormalTaus {
  float c[DPE_NORMAL_MAX_TAU];
  int n;
};

// st / tend: the cloud's finite points in bucket order and the buckets' ends; m: their number.  normal, count and sums
// (or null) are indexed by original index and were zeroed before (a non-finite point has no thread)
__global__ void __launch_bounds__(kNormalBlock) k_cloud_normal(const float4* __restrict__ st, int m, const int* __restrict__ tend,
                                                               CloudGrid g, double S, int min_nb, float* __restrict__ normal,
                                                               int* __restrict__ count, long long* __restrict__ sums) {
  const size_t i = (size_t)blockIdx.x * kNormalBlock + threadIdx.x;
  if (i >= (size_t)m) return;
  const float4 q = st[i];
  const NormalWalk w = normal_walk(g, q.x, q.y, q.z);
  long long s[kNormalSums] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < 27; ++k) {
    int32_t ix, iy, iz;
    if (!normal_cell(w, k, ix, iy, iz)) continue;
    const uint32_t b = cloud_bucket(ix, iy, iz, g.mask);
    if (normal_bucket_seen(w, g.mask, k, b)) continue;
    const int j1 = tend[b];
    for (int j = b ? tend[b - 1] : 0; j < j1; ++j) {
      const float4 t = st[j];
      if (cloud_d2(q.x, q.y, q.z, t.x, t.y, t.z) < g.r2) normal_add(q.x, q.y, q.z, t.x, t.y, t.z, S, s);
    }
  }
  float n[3];
  normal_solve(s, (long long)min_nb, n);
  const size_t at = (size_t)__float_as_int(q.w);
  normal[3 * at] = n[0];
  normal[3 * at + 1] = n[1];
  normal[3 * at + 2] = n[2];
  count[at] = (int)s[0];
  if (sums) {
#pragma unroll
    for (int e = 0; e < kNormalSums; ++e) sums[at * kNormalSums + e] = s[e];
  }
}

__global__ void __launch_bounds__(kNormalBlock) k_render_clear64(unsigned long long* __restrict__ zb, size_t npx) {
  const size_t i = (size_t)blockIdx.x * kNormalBlock + threadIdx.x;
  if (i < npx) zb[i] = kNormalEmptyWord;
}

__global__ void __launch_bounds__(kNormalBlock) k_render_splat_idx(const float* __restrict__ pts, int n, DpeCamera cam, int s,
                                                                   unsigned long long* zb) {
  const size_t i = (size_t)blockIdx.x * kNormalBlock + threadIdx.x;
  if (i >= (size_t)n) return;
  int cx, cy;
  uint32_t z;
  if (!depth_point(cam, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], cx, cy, z)) return;
  const unsigned long long word = normal_word(z, (uint32_t)i);
  const int w = cam.width, h = cam.height;
  const int x0 = cx - s < 0 ? 0 : cx - s, x1 = cx + s > w - 1 ? w - 1 : cx + s;
  const int y0 = cy - s < 0 ? 0 : cy - s, y1 = cy + s > h - 1 ? h - 1 : cy + s;
  for (int y = y0; y <= y1; ++y) {
    unsigned long long* row = zb + (size_t)y * (size_t)w;
    for (int x = x0; x <= x1; ++x)
      if (word < __atomic_load_n(row + x, __ATOMIC_RELAXED)) atomicMin(row + x, word);
  }
}

__global__ void __launch_bounds__(kNormalBlock) k_render_finish_idx(const unsigned long long* __restrict__ zb, size_t npx,
                                                                    uint32_t* __restrict__ map, int* __restrict__ winner) {
  const size_t i = (size_t)blockIdx.x * kNormalBlock + threadIdx.x;
  if (i >= npx) return;
  const unsigned long long word = zb[i];
  const uint32_t z = (uint32_t)(word >> 32);
  const bool empty = z == kDepthEmpty;
  map[i] = empty ? 0u : z;
  winner[i] = empty ? -1 : (int)(uint32_t)word;
}

// pts / normals: the staged scan and its normals, f32 [n][3]; out: the normal map f32 [npx][3]
__global__ void __launch_bounds__(kNormalBlock) k_render_normals(const float* __restrict__ pts, const float* __restrict__ normals,
                                                                 const int* __restrict__ winner, size_t npx, DpeCamera cam,
                                                                 float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kNormalBlock + threadIdx.x;
  if (i >= npx) return;
  float o[3] = {0.0f, 0.0f, 0.0f};
  const int j = winner[i];
  if (j >= 0) {
    const size_t at = 3 * (size_t)j;
    const float n[3] = {normals[at], normals[at + 1], normals[at + 2]};
    if (!normal_none(n[0], n[1], n[2])) normal_orient(cam, pts[at], pts[at + 1], pts[at + 2], n, o);
  }
  out[3 * i] = o[0];
  out[3 * i + 1] = o[1];
  out[3 * i + 2] = o[2];
}

// edges: the 180 bin edges; part: 2 doubles per block; counts: kNormalCounters words; err: the error map or null
__global__ void __launch_bounds__(kNormalBlock) k_normal_score(const float* __restrict__ est, const float* __restrict__ gt,
                                                               size_t npx, NormalTaus T, const float* __restrict__ edges,
                                                               double* __restrict__ part, unsigned long long* __restrict__ counts,
                                                               float* __restrict__ err) {
  __shared__ int wc[kNormalBlock / 64][3 + DPE_NORMAL_MAX_TAU];
  __shared__ float E[kNormalBins];
  __shared__ unsigned int hist[kNormalBins];
  if ((int)threadIdx.x < kNormalBins) { E[threadIdx.x] = edges[threadIdx.x]; hist[threadIdx.x] = 0u; }
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * kNormalBlock + threadIdx.x;
  const bool in = i < npx;
  float e[3] = {0.0f, 0.0f, 0.0f}, g[3] = {0.0f, 0.0f, 0.0f};   // past the end: neither has a normal
  if (in) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { e[a] = est[3 * i + a]; g[a] = gt[3 * i + a]; }
  }
  const NormalPixel p = normal_pixel(e[0], e[1], e[2], g[0], g[1], g[2]);
  double t[kNormalTerms];
  normal_terms(p, t);
  if (in && err) err[i] = normal_error_code(p);
  if (p.both) atomicAdd(&hist[normal_bin(E, p.c)], 1u);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c_gt = __popcll(__ballot(p.gt_ok)), c_est = __popcll(__ballot(p.est_ok)), c_both = __popcll(__ballot(p.both));
  if (lane == 0) { wc[wave][0] = c_gt; wc[wave][1] = c_est; wc[wave][2] = c_both; }
  for (int k = 0; k < T.n; ++k) {
    const int c = __popcll(__ballot(p.both && p.c > T.c[k]));
    if (lane == 0) wc[wave][3 + k] = c;
  }
  block_tree_sum<kNormalTerms>(t, part + (size_t)blockIdx.x * kNormalTerms);   // its barrier also publishes wc and hist
  if ((int)threadIdx.x < 3 + T.n) {
    const int k = threadIdx.x;
    const int all = wc[0][k] + wc[1][k] + wc[2][k] + wc[3][k];
    if (all > 0) atomicAdd(counts + k, (unsigned long long)all);
  }
  if ((int)threadIdx.x < kNormalBins) {
    const unsigned int v = hist[threadIdx.x];
    if (v > 0u) atomicAdd(counts + 3 + DPE_NORMAL_MAX_TAU + threadIdx.x, (unsigned long long)v);
  }
}

}  // namespace dpe
