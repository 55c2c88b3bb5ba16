// cloud_dist.h — the arithmetic of the cloud evaluation that the host (host/cloud_eval.cpp) shares with the
// kernels (pass_cloud.h): the squared distance of the contract, the cell of a point and the bucket of a
// cell.  Plain C++, single precision where the contract says so, -ffp-contract=off like everything here.
//
// The grid.  Cell edge h = max(R, 2^-62) * (1 + 2^-10) in double; origin o = the per-axis minimum of the
// finite target points; cell(x) = floor(((double)x - (double)o) / h), one int32 per axis.  A query visits
// the 27 cells around its own.
//
// Coverage (every t with s = d2(q, t) < R2 lies in those 27 cells).  s is a sum of non-negative terms under
// six roundings, so s >= (qx - tx)^2 * (1 - 2^-21) per axis (R2 subnormal: every term is below 2^-126, so
// |qx - tx| < 2^-62, which is why h has that floor), and R2 <= R^2 * (1 + 2^-24): s < R2 gives
// |qx - tx| < R * (1 + 2^-20) per axis.  The computed cell coordinate u = (x - o) / h carries two double
// roundings, at most 2^-21 in absolute terms while u < 2^30 (kCloudMaxCell), so |u_q - u_t| <
// (1 + 2^-20) / (1 + 2^-10) + 2^-20 < 1, and two numbers less than 1 apart have floors at most 1 apart.
//
// The limit: a target cell coordinate of kCloudMaxCell or more ("radius too small for the cloud's extent")
// is refused before any conversion to int.  A query may lie anywhere: its coordinate is clamped to
// [-2, max target cell + 2] in double first; a cell that far out has no target in its 27 neighbours, and
// neither has the cell it is clamped to.
//
// Buckets: nb a power of two, bucket = hash(cell) & (nb - 1).  Cells that share a bucket only add
// candidates; the exact d2 decides.
#pragma once
#include <stdint.h>

#include "chd.h"   // DPE_CHD

namespace dpe {

constexpr double kCloudMaxCell = 1073741824.0;   // 2^30: target cell coordinates lie in [0, 2^30)

// the contract's d2: every operation rounded to float, in this order
DPE_CHD float cloud_d2(float qx, float qy, float qz, float tx, float ty, float tz) {
  const float dx = qx - tx, dy = qy - ty, dz = qz - tz;
  float s = dx * dx;
  s = s + dy * dy;
  s = s + dz * dz;
  return s;
}

DPE_CHD bool cloud_finite(float v) {
  union { float f; uint32_t u; } b;
  b.f = v;
  return (b.u & 0x7F800000u) != 0x7F800000u;
}
DPE_CHD bool cloud_finite3(float x, float y, float z) { return cloud_finite(x) && cloud_finite(y) && cloud_finite(z); }

// the grid of one target cloud; filled by the host from the target's bounds (cloud_grid_make)
struct CloudGrid {
  double o[3];      // origin: per-axis minimum of the finite target points
  double h;         // cell edge
  double hi[3];     // largest target cell coordinate per axis, as a double
  uint32_t mask;    // nb - 1
  float r2;         // R * R in float
};

DPE_CHD double cloud_cell_edge(float radius) {
  const double r = (double)radius < 0x1p-62 ? 0x1p-62 : (double)radius;
  return r * (1.0 + 0x1p-10);
}

// the cell of a finite x on one axis: the coordinate clamped to [-2, hi + 2] in double, then its floor
// as an int32 (a target's coordinate lies in [0, hi] and is never clamped)
DPE_CHD int32_t cloud_cell(float x, double origin, double h, double hi) {
  const double u = ((double)x - origin) / h;
  if (!(u > -2.0)) return -2;
  if (!(u < hi + 2.0)) return (int32_t)hi + 2;
  const long long f = (long long)u;
  return (int32_t)((double)f > u ? f - 1 : f);
}

DPE_CHD uint32_t cloud_bucket(int32_t ix, int32_t iy, int32_t iz, uint32_t mask) {
  return (((uint32_t)ix * 73856093u) ^ ((uint32_t)iy * 19349663u) ^ ((uint32_t)iz * 83492791u)) & mask;
}

DPE_CHD uint32_t cloud_bucket_of(const CloudGrid& g, float x, float y, float z) {
  return cloud_bucket(cloud_cell(x, g.o[0], g.h, g.hi[0]), cloud_cell(y, g.o[1], g.h, g.hi[1]),
                      cloud_cell(z, g.o[2], g.h, g.hi[2]), g.mask);
}

// Buckets for m finite target points: the power of two at or above m / 4, between 64 and 2^28.
inline uint32_t cloud_bucket_count(size_t m) {
  uint32_t nb = 64;
  while (nb < (1u << 28) && (size_t)nb * 4 < m) nb <<= 1;
  return nb;
}

// The grid of a target cloud with finite bounds lo[3] <= hi[3] (float).  False: a cell coordinate would
// reach kCloudMaxCell.
inline bool cloud_grid_make(const float lo[3], const float hi[3], size_t m, float radius, CloudGrid* g) {
  g->h = cloud_cell_edge(radius);
  g->r2 = radius * radius;
  g->mask = cloud_bucket_count(m) - 1;
  for (int a = 0; a < 3; ++a) {
    g->o[a] = (double)lo[a];
    const double u = ((double)hi[a] - (double)lo[a]) / g->h;
    if (!(u < kCloudMaxCell)) return false;
    g->hi[a] = (double)(long long)u;   // u >= 0: truncation is floor
  }
  return true;
}

// ---- voxel down-sampling (dpe_cloud_voxel of include/dpe_mvs.h, which states the contract; the kernels are
// pass_voxel.h's, the serial loop host/cloud_voxel.cpp's).  A voxel is a cell of edge h = (double)v over the
// origin o = the per-axis minimum of the finite points.  Everything a record holds is a sum, a minimum or a
// count over the voxel's points in integers, so it does not depend on the order in which they are met.

// the voxel grid of a cloud; filled by the host from the cloud's bounds (voxel_grid_make)
struct VoxelGrid {
  double o[3];      // origin: per-axis minimum of the finite points
  double h;         // voxel edge
};

// The grid of a cloud with finite bounds lo[3] <= hi[3] (float).  False: the extent reaches kCloudMaxCell
// voxels on an axis (decided on the double, as cloud_grid_make does).
inline bool voxel_grid_make(const float lo[3], const float hi[3], float v, VoxelGrid* g) {
  g->h = (double)v;
  for (int a = 0; a < 3; ++a) {
    g->o[a] = (double)lo[a];
    const double u = ((double)hi[a] - (double)lo[a]) / g->h;
    if (!(u < kCloudMaxCell)) return false;
  }
  return true;
}

// Slots of the open-addressing table for m finite points: the power of two at or above 2 m, 64 at least and
// 2^31 at most (a slot index is kept in an int; m < 2^31, so even then the table is never full).
inline uint64_t voxel_slot_count(size_t m) {
  uint64_t s = 64;
  while (s < (1ull << 31) && s < 2 * (uint64_t)m) s <<= 1;
  return s;
}

// One axis of a finite point of the cloud the grid was made from: u = (x - o) / h in [0, 2^30) (cloud_cell's
// arithmetic, never clamped), *c = floor(u), and the return value q = (uint64)((u - c) * 2^32) truncated: the
// point's place inside the voxel on a lattice of 2^32 steps.  u - c is exact and lies in [0, 1), so q < 2^32.
DPE_CHD uint32_t voxel_cell_frac(float x, double origin, double h, int32_t* c) {
  const double u = ((double)x - origin) / h;
  const long long t = (long long)u;
  const long long fl = (double)t > u ? t - 1 : t;
  *c = (int32_t)fl;
  const double f = u - (double)fl;
  return (uint32_t)(unsigned long long)(f * 4294967296.0);
}

// The coordinate of a voxel's record on one axis from the integer sum S of its points' q: every operation a
// rounded double operation in this order, then one rounding to float.
DPE_CHD float voxel_coord(double origin, double h, int32_t c, unsigned long long S, int32_t count) {
  const double mean = (double)S / (double)count;
  const double t = mean * 0x1p-32;
  const double u = (double)c + t;
  const double w = u * h;
  return (float)(origin + w);
}

// The colour channel of a voxel's record from the 64-bit sum of its points' channel: the mean rounded half up.
DPE_CHD uint8_t voxel_colour(unsigned long long sum, int32_t count) {
  const unsigned long long n = (unsigned long long)count;
  return (uint8_t)((2ull * sum + n) / (2ull * n));
}

}  // namespace dpe
