// pass_points.h — ExportDepthImagePointCloud (DPE.cpp:1691-1724) on the GPU: one image's depth map
// back-projected into coloured points, in the reference's order.
//
// The reference walks `for i < cols, for j < rows`: COLUMN-major, unlike every other compaction here.
// A pixel's rank is the number of valid pixels in the columns before its own plus the valid pixels
// above it in its column.  The image is cut into cells of one column by kPtsSeg rows:
//
//   k_pts_count    one thread per cell: the valid pixels of the cell into cnt[column * nseg + segment],
//                  which is the order the reference visits the cells in
//   k_offsets_scan (block_scan.h) exclusive sum-scan of cnt in that order (one block), the image's total into *tot
//   k_pts_fill     one thread per cell again: its pixels top to bottom into out[cnt[cell]...]
//
// No atomics, so the order is the reference's whatever the schedule.  A block is kPtsCols adjacent
// columns of one segment and a thread keeps its column, so at every row the lanes of a wave read
// adjacent pixels of one image row: depth, pixel state and colour are read along the rows they are
// stored in, once for the counts and once for the fill.  The counts need no exchange between lanes.
//
// mode DPE_POINTS_STRONG (main.cpp:464): a pixel that is not STRONG has its depth REPLACED by 0 before
// the test, so with depth_min <= 0 it is emitted at depth 0, as the reference's code would.
// The test `depth < depth_min || depth > depth_max || isnan(depth)`: NaN on the bit pattern.
#pragma once
#include "block_scan.h"      // k_offsets_scan
#include "fusion_world.h"
#include "dpe_fusion_types.h"   // TatPoint (= DpeFusedPoint)

namespace dpe {

constexpr int kPtsCols = 256;   // columns per block
constexpr int kPtsSeg = 32;     // rows per cell

__device__ inline float pts_depth(int mode, const float4* __restrict__ planes, const uint8_t* __restrict__ weak, size_t p) {
  const float d = planes[p].w;
  return (mode == DPE_POINTS_STRONG && weak[p] != DPE_STRONG) ? 0.0f : d;
}

__device__ inline bool pts_valid(float d, float dmin, float dmax) {
  const bool is_nan = (__float_as_uint(d) & 0x7FFFFFFFu) > 0x7F800000u;
  return !(d < dmin || d > dmax || is_nan);
}

// grid (ceil(w / kPtsCols), nseg)
__global__ void __launch_bounds__(kPtsCols) k_pts_count(int mode, const float4* __restrict__ planes,
                                                        const uint8_t* __restrict__ weak, int w, int h, int nseg,
                                                        float dmin, float dmax, int* __restrict__ cnt) {
  const int c = blockIdx.x * kPtsCols + threadIdx.x;
  if (c >= w) return;
  const int seg = blockIdx.y;
  const int j0 = seg * kPtsSeg, j1 = min(h, j0 + kPtsSeg);
  int n = 0;
  for (int j = j0; j < j1; ++j)
    n += pts_valid(pts_depth(mode, planes, weak, (size_t)j * w + c), dmin, dmax) ? 1 : 0;
  cnt[(size_t)c * nseg + seg] = n;
}

// grid as k_pts_count; off = the scanned cnt.  Writes exactly the pixels k_pts_count counted.
__global__ void __launch_bounds__(kPtsCols) k_pts_fill(int mode, const float4* __restrict__ planes,
                                                       const uint8_t* __restrict__ weak, const uint8_t* __restrict__ bgr,
                                                       DpeCamera cam, int w, int h, int nseg, float dmin, float dmax,
                                                       const int* __restrict__ off, TatPoint* __restrict__ out) {
  const int c = blockIdx.x * kPtsCols + threadIdx.x;
  if (c >= w) return;
  const int seg = blockIdx.y;
  const int j0 = seg * kPtsSeg, j1 = min(h, j0 + kPtsSeg);
  int a = off[(size_t)c * nseg + seg];
  for (int j = j0; j < j1; ++j) {
    const size_t p = (size_t)j * w + c;
    const float d = pts_depth(mode, planes, weak, p);
    if (!pts_valid(d, dmin, dmax)) continue;
    const FP3 X = fz_world(c, j, d, cam);
    const uint8_t* col = bgr + 3 * p;
    out[a++] = TatPoint{X.x, X.y, X.z, (float)col[0], (float)col[1], (float)col[2]};
  }
}

}  // namespace dpe
