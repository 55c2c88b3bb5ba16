// pass_voxel.h — voxel down-sampling of a point cloud (dpe_cloud_voxel of include/dpe_mvs.h, which states the
// contract): one record per non-empty voxel, in ascending order of the voxel's first point, the bits of a
// serial loop.  The arithmetic is cloud_dist.h's, which the host path (host/cloud_voxel.cpp) shares; the
// bounds come from pass_cloud.h's k_cloud_bounds and the block offsets from its k_cloud_scan.
//
//   k_voxel_cells   per point its cell (3 x int32 and a valid flag) and its three lattice fractions
//   k_voxel_insert  an open-addressing table over the cells, linear probing from cloud_bucket: a thread claims
//                   a slot with one atomicCAS on owner[] and learns the owner from that call's return value
//                   alone; it compares its cell with the owner's, which the PREVIOUS launch wrote, so nothing
//                   is ordered inside the kernel.  On a match or a fresh claim: atomicMin on first[],
//                   atomicAdd on count[], three 64-bit integer adds of the fractions and three of the colours
//                   (a wave whose lanes all found one slot sums them first and adds once).  The loop is
//                   bounded by the slot count; exhausting it sets the error word.  No thread waits for another.
//   k_voxel_mark    every occupied slot writes its index to slot_at[first[slot]]
//   k_voxel_count   marked indices per block of kVoxelBlock points (ballot), then k_cloud_scan over the blocks
//   k_voxel_fill    stable fill by ballot over the original indices: the marked index of rank r computes
//                   record r from its slot's sums (voxel_coord, voxel_colour) and writes the four outputs
//
// Which slot a voxel gets depends on the schedule; a record is made of integer sums, a minimum and a count
// over the voxel's points and does not.  No float atomics, no LDS beyond the wave counts of count and fill,
// no scratch.  Sizes: points are int (< 2^31), slots at most 2^31; every element offset is formed in size_t.
#pragma once
#include <hip/hip_runtime.h>

#include "cloud_dist.h"

namespace dpe {

constexpr int kVoxelBlock = 256;
constexpr int kVoxelEmpty = -1;            // owner[] of a free slot (memset 0xFF)

// the table: owner and first start as 0xFF bytes, everything else as 0
struct VoxelTable {
  int* owner;                    // the point that claimed the slot, or kVoxelEmpty
  uint32_t* first;               // lowest original index of the slot's points (unsigned: starts at 2^32 - 1)
  int* count;
  unsigned long long* sum;       // [slot][3]: the lattice fractions' sums
  unsigned long long* csum;      // [slot][3]: the colour channels' sums (untouched without colours)
  uint32_t mask;                 // slots - 1
};

__global__ void __launch_bounds__(kVoxelBlock) k_voxel_cells(const float* __restrict__ pts, int n, VoxelGrid g,
                                                             int4* __restrict__ cell, uint32_t* __restrict__ frac) {
  const size_t i = (size_t)blockIdx.x * kVoxelBlock + threadIdx.x;
  if (i >= (size_t)n) return;
  const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
  int4 c = make_int4(0, 0, 0, 0);
  uint32_t q[3] = {0u, 0u, 0u};
  if (cloud_finite3(x, y, z)) {
    q[0] = voxel_cell_frac(x, g.o[0], g.h, &c.x);
    q[1] = voxel_cell_frac(y, g.o[1], g.h, &c.y);
    q[2] = voxel_cell_frac(z, g.o[2], g.h, &c.z);
    c.w = 1;
  }
  cell[i] = c;
  frac[3 * i] = q[0]; frac[3 * i + 1] = q[1]; frac[3 * i + 2] = q[2];
}

__global__ void __launch_bounds__(kVoxelBlock) k_voxel_insert(const int4* __restrict__ cell, const uint32_t* __restrict__ frac,
                                                              const uint8_t* __restrict__ rgb, int n, VoxelTable t,
                                                              uint32_t* __restrict__ err) {
  const size_t i = (size_t)blockIdx.x * kVoxelBlock + threadIdx.x;
  int4 c = make_int4(0, 0, 0, 0);
  if (i < (size_t)n) c = cell[i];
  uint32_t s = 0;
  bool found = false;
  if (c.w) {
    s = cloud_bucket(c.x, c.y, c.z, t.mask);
    for (uint64_t probe = 0; probe <= (uint64_t)t.mask; ++probe, s = (s + 1u) & t.mask) {
      const int prev = atomicCAS(&t.owner[s], kVoxelEmpty, (int)i);
      if (prev != kVoxelEmpty) {
        const int4 oc = cell[(size_t)prev];
        if (oc.x != c.x || oc.y != c.y || oc.z != c.z) continue;
      }
      found = true;
      break;
    }
    if (!found) atomicOr(err, 1u);
  }
  uint32_t lowest = found ? (uint32_t)i : 0xFFFFFFFFu;
  int cnt = found ? 1 : 0;
  unsigned long long q[3] = {0ull, 0ull, 0ull};
  uint32_t col[3] = {0u, 0u, 0u};
  if (found) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { q[a] = frac[3 * i + a]; if (rgb) col[a] = rgb[3 * i + a]; }
  }
  // every lane of the wave is here (the block is whole waves and nothing returned): when all the lanes that found
  // a slot found the SAME one, their contributions are summed in the wave and one lane adds them.  Raster-ordered
  // depth maps put neighbours in one voxel; measured interleaved against the kernel without this block
  // (profiles/cloud_voxel_ab.json): 0.75 -> 0.28 ms on 20 000 points of one voxel, 1 to 2 % less on 1.92 million points.
  const unsigned long long act = __ballot(found);
  if (act == 0ull) return;
  const int lead = __ffsll((long long)act) - 1;
  const uint32_t s0 = (uint32_t)__shfl((int)s, lead);
  if (__popcll(act) > 1 && __ballot(found && s == s0) == act) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      lowest = min(lowest, (uint32_t)__shfl_xor((int)lowest, o));
      cnt += __shfl_xor(cnt, o);
#pragma unroll
      for (int a = 0; a < 3; ++a) { q[a] += __shfl_xor(q[a], o); col[a] += (uint32_t)__shfl_xor((int)col[a], o); }
    }
    found = (int)(threadIdx.x & 63) == lead;
  }
  if (!found) return;
  atomicMin(&t.first[s], lowest);
  atomicAdd(&t.count[s], cnt);
#pragma unroll
  for (int a = 0; a < 3; ++a) atomicAdd(&t.sum[3 * (size_t)s + a], q[a]);
  if (rgb) {
#pragma unroll
    for (int a = 0; a < 3; ++a) atomicAdd(&t.csum[3 * (size_t)s + a], (unsigned long long)col[a]);
  }
}

// slot_at starts as -1 everywhere (memset 0xFF); a slot index fits an int (voxel_slot_count stops at 2^31)
__global__ void __launch_bounds__(kVoxelBlock) k_voxel_mark(VoxelTable t, int* __restrict__ slot_at) {
  const size_t s = (size_t)blockIdx.x * kVoxelBlock + threadIdx.x;
  if (s > (size_t)t.mask) return;
  if (t.owner[s] != kVoxelEmpty) slot_at[(size_t)t.first[s]] = (int)(uint32_t)s;
}

// marked indices before this thread's in its block, and (in *total) in the whole block
__device__ inline int voxel_block_rank(bool flag, int* s4, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long b = __ballot(flag);
  if (lane == 0) s4[wave] = __popcll(b);
  __syncthreads();
  int before = __popcll(b & ((1ull << lane) - 1ull)), all = 0;
#pragma unroll
  for (int v = 0; v < kVoxelBlock / 64; ++v) { if (v < wave) before += s4[v]; all += s4[v]; }
  *total = all;
  return before;
}

// bcnt[block] = the block's marked indices; bcnt has one entry more than there are blocks, left 0, so the
// exclusive scan puts the number of voxels there
__global__ void __launch_bounds__(kVoxelBlock) k_voxel_count(const int* __restrict__ slot_at, int n, int* __restrict__ bcnt) {
  __shared__ int s4[kVoxelBlock / 64];
  const size_t i = (size_t)blockIdx.x * kVoxelBlock + threadIdx.x;
  const bool flag = i < (size_t)n && slot_at[i] >= 0;
  int all;
  voxel_block_rank(flag, s4, &all);
  if (threadIdx.x == 0) bcnt[blockIdx.x] = all;
}

// boff: the scanned block counts
__global__ void __launch_bounds__(kVoxelBlock) k_voxel_fill(const int* __restrict__ slot_at, int n, const int* __restrict__ boff,
                                                            const int4* __restrict__ cell, VoxelGrid g, VoxelTable t,
                                                            float* __restrict__ out_xyz, uint8_t* __restrict__ out_rgb,
                                                            int* __restrict__ out_first, int* __restrict__ out_count) {
  __shared__ int s4[kVoxelBlock / 64];
  const size_t i = (size_t)blockIdx.x * kVoxelBlock + threadIdx.x;
  const int sl = i < (size_t)n ? slot_at[i] : -1;
  int all;
  const int before = voxel_block_rank(sl >= 0, s4, &all);
  if (sl < 0) return;
  const size_t r = (size_t)boff[blockIdx.x] + (size_t)before, s = (size_t)(uint32_t)sl;
  const int4 c = cell[i];
  const int cnt = t.count[s];
  out_xyz[3 * r] = voxel_coord(g.o[0], g.h, c.x, t.sum[3 * s], cnt);
  out_xyz[3 * r + 1] = voxel_coord(g.o[1], g.h, c.y, t.sum[3 * s + 1], cnt);
  out_xyz[3 * r + 2] = voxel_coord(g.o[2], g.h, c.z, t.sum[3 * s + 2], cnt);
  if (out_rgb) {
#pragma unroll
    for (int a = 0; a < 3; ++a) out_rgb[3 * r + a] = voxel_colour(t.csum[3 * s + a], cnt);
  }
  out_first[r] = (int)i;
  out_count[r] = cnt;
}

}  // namespace dpe
