// pass_register.h — the nearest neighbour with its index and one step of point-to-point ICP (dpe_cloud_nn_index
// and dpe_cloud_icp_step of include/dpe_mvs.h, which states the contract).  The grid and its build steps are
// pass_cloud.h's, the arithmetic is cloud_reg.h's, which the host path (host/cloud_register.cpp) shares.
//
//   k_icp_apply    one thread per source point: its image under T as f32; a non-finite source becomes NaN, so it
//                  goes to the queries' bucket 0 and matches nothing
//   k_icp_terms    block = 256 consecutive source indices: every thread forms its 16 terms (+0.0 without a match),
//                  the block sums them by the butterfly of tree_sum.h and adds its match count by one integer
//                  atomic; k_tree_reduce<16> takes the block results from there
//
// The match is k_cloud_match of pass_cloud.h.
#pragma once
#include <hip/hip_runtime.h>

#include "cloud_reg.h"
#include "pass_cloud.h"
#include "tree_sum.h"

namespace dpe {

struct IcpXf { double m[12]; };      // T, row-major 3 x 4
struct IcpOrigins { double s[3], t[3]; };   // per-axis minima of the finite source / target points

__global__ void __launch_bounds__(kCloudBlock) k_icp_apply(const float* __restrict__ src, int n, IcpXf T,
                                                           float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kCloudBlock + threadIdx.x;
  if (i >= (size_t)n) return;
  const float x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
  float o[3] = {__int_as_float(0x7FC00000), __int_as_float(0x7FC00000), __int_as_float(0x7FC00000)};
  if (cloud_finite3(x, y, z)) icp_apply(T.m, x, y, z, o);
  out[3 * i] = o[0]; out[3 * i + 1] = o[1]; out[3 * i + 2] = o[2];
}

// part: 16 doubles per block; count: the matched sources (one atomic per block)
__global__ void __launch_bounds__(kCloudBlock) k_icp_terms(const float* __restrict__ src, int n, const float* __restrict__ tgt,
                                                           const int* __restrict__ idx, const float* __restrict__ d2,
                                                           IcpOrigins o, double* __restrict__ part,
                                                           unsigned long long* __restrict__ count) {
  __shared__ int hits[kCloudBlock / 64];
  const size_t i = (size_t)blockIdx.x * kCloudBlock + threadIdx.x;
  double t[kIcpTerms];
#pragma unroll
  for (int k = 0; k < kIcpTerms; ++k) t[k] = 0.0;
  const int j = i < (size_t)n ? idx[i] : -1;
  if (j >= 0) {
    const float p[3] = {src[3 * i], src[3 * i + 1], src[3 * i + 2]};
    const size_t at = 3 * (size_t)j;
    const float g[3] = {tgt[at], tgt[at + 1], tgt[at + 2]};
    icp_terms(p, g, d2[i], o.s, o.t, t);
  }
  const int wave_hits = __popcll(__ballot(j >= 0));
  if ((threadIdx.x & 63) == 0) hits[threadIdx.x >> 6] = wave_hits;
  block_tree_sum<kIcpTerms>(t, part + (size_t)blockIdx.x * kIcpTerms);   // its barrier also publishes hits
  if (threadIdx.x == 0) {
    const int all = hits[0] + hits[1] + hits[2] + hits[3];
    if (all > 0) atomicAdd(count, (unsigned long long)all);
  }
}

}  // namespace dpe
