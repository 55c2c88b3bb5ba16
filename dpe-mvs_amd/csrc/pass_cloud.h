// pass_cloud.h — the truncated nearest-neighbour distance between two point clouds (dpe_cloud_nn of
// include/dpe_mvs.h): out[i] = min(R2, min_j d2(Q[i], T[j])), the bits of a serial loop.  The arithmetic,
// the grid and the argument why 27 cells cover every t with d2 < R2 are cloud_dist.h's, which the host path
// (host/cloud_eval.cpp) shares.
//
//   k_cloud_bounds  per-axis minimum and maximum of a cloud's finite points and their number (order-
//                   preserving integer keys, one integer atomic per wave and slot)
//   k_cloud_count   points per bucket (integer atomics); a non-finite point is left out of a target and
//                   goes to bucket 0 of a query
//   k_cloud_scan    exclusive sum-scan of the bucket counts in place (one block)
//   k_cloud_fill    every point into its bucket's next free slot, as (x, y, z, original index); the scanned
//                   counts advance to the buckets' ends
//   k_cloud_query   one thread per query in BUCKET order, so the lanes of a wave mostly share their 27
//                   neighbour cells and read the same target points: the running minimum over the buckets
//                   of those cells, written back by original index
//   k_cloud_match   the same walk with the running pair (best, best_j), for the registration (pass_register.h)
//
// The target and the query go through the same three build steps over the same grid.  The slots within a
// bucket depend on the schedule; the result is a minimum over a set and does not.  No LDS and no scratch.
// Sizes: points and buckets are int (< 2^31); every element offset is formed in size_t.
#pragma once
#include <hip/hip_runtime.h>

#include "cloud_dist.h"
#include "cloud_reg.h"     // icp_take
#include "tree_sum.h"      // kTreeBlock
#include "block_scan.h"

namespace dpe {

constexpr int kCloudBlock = kTreeBlock;
constexpr int kCloudScanPer = 8;   // counts per thread and round of k_cloud_scan

// keys whose unsigned order is the floats' order (finite values)
__device__ inline uint32_t cloud_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// b[0..2] the INVERTED minimum keys, b[3..5] the maximum keys, b[6] the finite points: all maxima or sums
// that start at 0, so one memset prepares them
__global__ void __launch_bounds__(kCloudBlock) k_cloud_bounds(const float* __restrict__ pts, int n, uint32_t* __restrict__ b) {
  uint32_t lo[3] = {0u, 0u, 0u}, hi[3] = {0u, 0u, 0u}, cnt = 0;   // lo: inverted keys
  for (size_t i = (size_t)blockIdx.x * kCloudBlock + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * kCloudBlock) {
    const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    if (!cloud_finite3(x, y, z)) continue;
    const uint32_t k[3] = {cloud_key(x), cloud_key(y), cloud_key(z)};
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = max(lo[a], ~k[a]); hi[a] = max(hi[a], k[a]); }
    ++cnt;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = max(lo[a], (uint32_t)__shfl_xor((int)lo[a], o));
      hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], o));
    }
    cnt += (uint32_t)__shfl_xor((int)cnt, o);
  }
  if ((threadIdx.x & 63) == 0 && cnt > 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { atomicMax(&b[a], lo[a]); atomicMax(&b[3 + a], hi[a]); }
    atomicAdd(&b[6], cnt);
  }
}

// the bucket of point i, or -1 for a non-finite point that is left out
__device__ inline int cloud_point_bucket(const float* __restrict__ pts, size_t i, const CloudGrid& g, int keep_nonfinite,
                                         float& x, float& y, float& z) {
  x = pts[3 * i]; y = pts[3 * i + 1]; z = pts[3 * i + 2];
  if (!cloud_finite3(x, y, z)) return keep_nonfinite ? 0 : -1;
  return (int)cloud_bucket_of(g, x, y, z);
}

__global__ void __launch_bounds__(kCloudBlock) k_cloud_count(const float* __restrict__ pts, int n, CloudGrid g,
                                                             int keep_nonfinite, int* __restrict__ cnt) {
  const size_t i = (size_t)blockIdx.x * kCloudBlock + threadIdx.x;
  if (i >= (size_t)n) return;
  float x, y, z;
  const int b = cloud_point_bucket(pts, i, g, keep_nonfinite, x, y, z);
  if (b >= 0) atomicAdd(&cnt[b], 1);
}

// exclusive scan of cnt[0..nb) in place, one block: a thread sums kCloudScanPer adjacent counts, the
// block scans the threads' sums (block_scan.h), and a carry runs over the rounds
__global__ void __launch_bounds__(kCloudBlock) k_cloud_scan(int nb, int* __restrict__ cnt) {
  static_assert(kCloudBlock == kScanBlock, "block_scan scans 256 threads");
  __shared__ int s4[4];
  int acc = 0;
  for (size_t k0 = 0; k0 < (size_t)nb; k0 += (size_t)kCloudBlock * kCloudScanPer) {
    const size_t k = k0 + (size_t)threadIdx.x * kCloudScanPer;
    int c[kCloudScanPer], sum = 0;
#pragma unroll
    for (int e = 0; e < kCloudScanPer; ++e) { c[e] = k + e < (size_t)nb ? cnt[k + e] : 0; sum += c[e]; }
    int all;
    int run = acc + block_scan<ScanSum>(sum, s4, &all) - sum;
#pragma unroll
    for (int e = 0; e < kCloudScanPer; ++e) { if (k + e < (size_t)nb) cnt[k + e] = run; run += c[e]; }
    acc += all;
  }
}

// cur: the scanned counts; after the kernel cur[b] is the END of bucket b (its start is cur[b - 1], or 0)
__global__ void __launch_bounds__(kCloudBlock) k_cloud_fill(const float* __restrict__ pts, int n, CloudGrid g,
                                                            int keep_nonfinite, int* __restrict__ cur,
                                                            float4* __restrict__ sorted) {
  const size_t i = (size_t)blockIdx.x * kCloudBlock + threadIdx.x;
  if (i >= (size_t)n) return;
  float x, y, z;
  const int b = cloud_point_bucket(pts, i, g, keep_nonfinite, x, y, z);
  if (b < 0) return;
  const int slot = atomicAdd(&cur[b], 1);
  sorted[slot] = make_float4(x, y, z, __int_as_float((int)i));
}

// The walk of one query over the 27 cells around its own (cloud_dist.h says why they are enough), as the host
// writes it (cloud_query_range, host/cloud_eval.cpp).  The caller starts best at R2 and best_j at -1; best ends as
// min(R2, min_j d2), and with kIndex the running pair (best, best_j) as the lexicographic minimum of (d2, j), a
// set's minimum whatever the slots' order.
// st / tend: the target's points in bucket order and the buckets' ends
template <bool kIndex>
__device__ inline void cloud_walk(const float4 q, const float4* __restrict__ st, const int* __restrict__ tend,
                                  const CloudGrid& g, float& best, int& best_j) {
  if (!cloud_finite3(q.x, q.y, q.z)) return;
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
          const float s = cloud_d2(q.x, q.y, q.z, t.x, t.y, t.z);
          if constexpr (kIndex) icp_take(s, __float_as_int(t.w), best, best_j);
          else best = s < best ? s : best;
        }
      }
    }
  }
}

// sq: the n queries in bucket order; the distances are written back by original index
__global__ void __launch_bounds__(kCloudBlock) k_cloud_query(const float4* __restrict__ sq, int n, const float4* __restrict__ st,
                                                             const int* __restrict__ tend, CloudGrid g,
                                                             float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kCloudBlock + threadIdx.x;
  if (i >= (size_t)n) return;
  const float4 q = sq[i];
  float best = g.r2;
  int best_j = -1;
  cloud_walk<false>(q, st, tend, g, best, best_j);
  out[(size_t)__float_as_int(q.w)] = best;
}

// k_cloud_query with the nearest point's index (dpe_cloud_nn_index, the ICP step's match)
__global__ void __launch_bounds__(kCloudBlock) k_cloud_match(const float4* __restrict__ sq, int n, const float4* __restrict__ st,
                                                             const int* __restrict__ tend, CloudGrid g,
                                                             float* __restrict__ out, int* __restrict__ idx) {
  const size_t i = (size_t)blockIdx.x * kCloudBlock + threadIdx.x;
  if (i >= (size_t)n) return;
  const float4 q = sq[i];
  float best = g.r2;
  int best_j = -1;
  cloud_walk<true>(q, st, tend, g, best, best_j);
  const size_t at = (size_t)__float_as_int(q.w);
  out[at] = best;
  idx[at] = best_j;
}

}  // namespace dpe
