// pass_normals.h — the normal-map evaluation's own kernels (dpe_cloud_normals and dpe_cloud_render_view_normals of
// include/dpe_mvs.h, which states the contract).  The arithmetic is normal_eval.h's, which the host loops
// (host/normal_eval.cpp) share.
//
//   k_cloud_normal        one thread per finite point in BUCKET order over the grid that k_cloud_count / _scan / _fill
//                         built from the same cloud: cloud_walk's 27 cells, but the ten int64 sums instead of a minimum,
//                         then the 3 x 3 solve in the same thread; written back by original index.  NO POINT TWICE: a
//                         cell whose bucket an earlier cell of the 27 already gave is skipped (normal_eval.h says why
//                         that counts every neighbour exactly once)
//   k_render_finish_idx   one thread per pixel: the 64-bit word of k_render_splat<unsigned long long> split into the
//                         f32 map and the i32 winner, -1 where empty
//   k_render_normals      one thread per pixel: the winner's normal turned towards the camera, zeros without one
// The clear, the splat and the score are pass_render.h's templates.
//
// No float atomics, no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include "normal_eval.h"
#include "tree_sum.h"

namespace dpe {

constexpr int kNormalBlock = kTreeBlock;
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

}  // namespace dpe
