// pass_register.h — the nearest neighbour with its index and one step of point-to-point ICP (dpe_cloud_nn_index
// and dpe_cloud_icp_step of include/dpe_mvs.h, which states the contract).  The grid and its build steps are
// pass_cloud.h's, the arithmetic is cloud_reg.h's, which the host path (host/cloud_register.cpp) shares.
//
//   k_icp_apply    one thread per source point: its image under T as f32; a non-finite source becomes NaN, so it
//                  goes to the queries' bucket 0 and matches nothing
//   k_cloud_match  k_cloud_query with the running pair (best, best_j): the lexicographic minimum of (d2, j) over
//                  the 27 cells' buckets, a set's minimum whatever the slots' order; written back by original index
//   k_icp_terms    block = 256 consecutive source indices: every thread forms its 16 terms (+0.0 without a match),
//                  the block sums them by the xor butterfly (six levels inside a wave, two over the four waves
//                  through LDS as (w0 + w1) + (w2 + w3)) and adds its match count by one integer atomic
//   k_icp_reduce   the same butterfly over 256 consecutive partials, launched until one block's result is left
//
// The butterfly.  At level o = 1, 2, .. 32 a lane adds its partner's value (lane ^ o) to its own; addition is
// commutative, so both lanes of a pair hold the node s[2k] + s[2k + 1] of the contract's tree, and lanes past the
// end hold +0.0, the tree's missing right operand.  256 consecutive leaves are a complete subtree, so the levels
// over the block results continue the same tree.  No float atomics, no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include "cloud_reg.h"
#include "pass_cloud.h"

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

// sq: the n queries in bucket order; st / tend: the target's points in bucket order and the buckets' ends
__global__ void __launch_bounds__(kCloudBlock) k_cloud_match(const float4* __restrict__ sq, int n, const float4* __restrict__ st,
                                                             const int* __restrict__ tend, CloudGrid g,
                                                             float* __restrict__ out, int* __restrict__ idx) {
  const size_t i = (size_t)blockIdx.x * kCloudBlock + threadIdx.x;
  if (i >= (size_t)n) return;
  const float4 q = sq[i];
  float best = g.r2;
  int best_j = -1;
  if (cloud_finite3(q.x, q.y, q.z)) {
    const int32_t c[3] = {cloud_cell(q.x, g.o[0], g.h, g.hi[0]), cloud_cell(q.y, g.o[1], g.h, g.hi[1]),
                          cloud_cell(q.z, g.o[2], g.h, g.hi[2])};
    const int32_t top[3] = {(int32_t)g.hi[0], (int32_t)g.hi[1], (int32_t)g.hi[2]};
    for (int dz = -1; dz <= 1; ++dz) {
      const int32_t iz = c[2] + dz;
      if (iz < 0 || iz > top[2]) continue;
      for (int dy = -1; dy <= 1; ++dy) {
        const int32_t iy = c[1] + dy;
        if (iy < 0 || iy > top[1]) continue;
        for (int dx = -1; dx <= 1; ++dx) {
          const int32_t ix = c[0] + dx;
          if (ix < 0 || ix > top[0]) continue;
          const uint32_t b = cloud_bucket(ix, iy, iz, g.mask);
          const int j1 = tend[b];
          for (int j = b ? tend[b - 1] : 0; j < j1; ++j) {
            const float4 t = st[j];
            icp_take(cloud_d2(q.x, q.y, q.z, t.x, t.y, t.z), __float_as_int(t.w), best, best_j);
          }
        }
      }
    }
  }
  const size_t at = (size_t)__float_as_int(q.w);
  out[at] = best;
  idx[at] = best_j;
}

// a double from lane ^ o, moved as its two halves
__device__ inline double icp_shfl_xor(double v, int o) {
  const int lo = __shfl_xor(__double2loint(v), o), hi = __shfl_xor(__double2hiint(v), o);
  return __hiloint2double(hi, lo);
}

// t[0..16) of the 256 threads of a block summed by the butterfly; thread 0 writes the 16 sums to out
__device__ inline void icp_block_sum(double* t, double* __restrict__ out) {
  __shared__ double part[kCloudBlock / 64][kIcpTerms];
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
    for (int k = 0; k < kIcpTerms; ++k) t[k] = t[k] + icp_shfl_xor(t[k], o);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kIcpTerms; ++k) part[wave][k] = t[k];
  }
  __syncthreads();
  if (threadIdx.x < kIcpTerms) {
    const int k = threadIdx.x;
    const double left = part[0][k] + part[1][k], right = part[2][k] + part[3][k];
    out[k] = left + right;
  }
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
  icp_block_sum(t, part + (size_t)blockIdx.x * kIcpTerms);   // its barrier also publishes hits
  if (threadIdx.x == 0) {
    const int all = hits[0] + hits[1] + hits[2] + hits[3];
    if (all > 0) atomicAdd(count, (unsigned long long)all);
  }
}

// in: cnt partials of 16 doubles; out: one per block of 256 of them
__global__ void __launch_bounds__(kCloudBlock) k_icp_reduce(const double* __restrict__ in, int cnt, double* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kCloudBlock + threadIdx.x;
  double t[kIcpTerms];
#pragma unroll
  for (int k = 0; k < kIcpTerms; ++k) t[k] = i < (size_t)cnt ? in[i * kIcpTerms + k] : 0.0;
  icp_block_sum(t, out + (size_t)blockIdx.x * kIcpTerms);
}

}  // namespace dpe
