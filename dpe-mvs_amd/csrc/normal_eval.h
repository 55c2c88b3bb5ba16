// normal_eval.h — the arithmetic of the normal-map evaluation (dpe_cloud_normals, dpe_cloud_render_view_normals and
// dpe_normal_score of include/dpe_mvs.h, which states the contract) that the host (host/normal_eval.cpp) shares with
// the kernels (pass_normals.h): what one neighbour adds to the ten integer sums, the normal from those sums, the
// orientation of a rendered normal and what one pixel contributes to a score.  Plain C++, -ffp-contract=off like
// everything here: every operation below is one rounded operation, IEEE division and square root.
//
// No point counted twice.  A walk over the 27 cells around a query reads whole BUCKETS, and two of the 27 cells can
// hash to one bucket.  The remedy here: a cell whose bucket an earlier cell of the 27 already gave is skipped
// (normal_bucket_seen).  The first visit of a bucket meets all its points, those of the later cell included; points
// of cells outside the 27 fail d2 < R2 (cloud_dist.h's coverage argument read backwards), so every point of the
// neighbour set is counted exactly once.  A minimum does not care (cloud_walk); a sum does.
#pragma once
#include "../../include/dpe_mvs.h"
#include "cloud_dist.h"   // DPE_CHD, cloud_finite3, cloud_bucket
#include "depth_eval.h"   // depth_bits, depth_ok

#include <cmath>

namespace dpe {

constexpr int kNormalSums = 10;     // count, 3 first moments, 6 second moments
constexpr int kNormalSweeps = 8;    // cyclic Jacobi sweeps of the 3 x 3 solve, always all of them
constexpr int kNormalTerms = 2;     // 1 - c and its square
constexpr int kNormalBins = DPE_NORMAL_BINS;
constexpr int kNormalMinNb = 3;

// S of the contract: lattice steps per unit length, one rounded division
DPE_CHD double normal_scale(float radius) { return 32768.0 / (double)radius; }

// the walk of one query: its own cell c and the grid's largest cell coordinates top, per axis
struct NormalWalk {
  int32_t cx, cy, cz, tx, ty, tz;
};

// cell k = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1) of the 27 around the query's: its coordinates, false when it lies
// outside the grid's cells [0, top]
DPE_CHD bool normal_cell(const NormalWalk& w, int k, int32_t& ix, int32_t& iy, int32_t& iz) {
  iz = w.cz + k / 9 - 1;
  iy = w.cy + (k / 3) % 3 - 1;
  ix = w.cx + k % 3 - 1;
  return ix >= 0 && ix <= w.tx && iy >= 0 && iy <= w.ty && iz >= 0 && iz <= w.tz;
}

// true when a cell before k of the walk (one inside the grid) gave bucket b already
DPE_CHD bool normal_bucket_seen(const NormalWalk& w, uint32_t mask, int k, uint32_t b) {
  for (int e = 0; e < k; ++e) {
    int32_t ix, iy, iz;
    if (normal_cell(w, e, ix, iy, iz) && cloud_bucket(ix, iy, iz, mask) == b) return true;
  }
  return false;
}

// the walk of the finite point (x, y, z) over grid g
DPE_CHD NormalWalk normal_walk(const CloudGrid& g, float x, float y, float z) {
  NormalWalk w;
  w.cx = cloud_cell(x, g.o[0], g.h, g.hi[0]);
  w.cy = cloud_cell(y, g.o[1], g.h, g.hi[1]);
  w.cz = cloud_cell(z, g.o[2], g.h, g.hi[2]);
  w.tx = (int32_t)g.hi[0];
  w.ty = (int32_t)g.hi[1];
  w.tz = (int32_t)g.hi[2];
  return w;
}

// one neighbour t of q with d2(q, t) < R2 into the ten sums.  |k| <= 2^15 + 1, so k and every product fit an int32
DPE_CHD void normal_add(float qx, float qy, float qz, float tx, float ty, float tz, double S, long long* s) {
  const float dx = qx - tx, dy = qy - ty, dz = qz - tz;
  const int32_t kx = (int32_t)((double)dx * S), ky = (int32_t)((double)dy * S), kz = (int32_t)((double)dz * S);
  s[0] += 1;
  s[1] += kx; s[2] += ky; s[3] += kz;
  s[4] += kx * kx; s[5] += kx * ky; s[6] += kx * kz;
  s[7] += ky * ky; s[8] += ky * kz; s[9] += kz * kz;
}

// one Jacobi rotation of the pair (p, q) of a symmetric 3 x 3 matrix, r the third index: app, aqq, apq the pair's
// entries, arp, arq the third row's; (v0p, v0q) .. (v2p, v2q) the two columns of V.  cloud_register.cpp's formulas
DPE_CHD void normal_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                           double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double mag = theta < 0.0 ? -theta : theta;
  double t = 1.0 / (mag + __builtin_sqrt(theta * theta + 1.0));   // theta^2 = inf gives t = 0
  if (theta < 0.0) t = -t;
  const double c = 1.0 / __builtin_sqrt(t * t + 1.0), s = t * c;
  const double h = t * apq;
  app = app - h;
  aqq = aqq + h;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
  const double a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
  v0p = c * a0 - s * b0; v0q = s * a0 + c * b0;
  v1p = c * a1 - s * b1; v1q = s * a1 + c * b1;
  v2p = c * a2 - s * b2; v2q = s * a2 + c * b2;
}

// The normal of a point from its ten sums: false (and n = 0, 0, 0) when it has none.
DPE_CHD bool normal_solve(const long long* s, long long min_nb, float n[3]) {
  n[0] = n[1] = n[2] = 0.0f;
  if (s[0] < min_nb || s[0] < 1) return false;
  const double cnt = (double)s[0], sx = (double)s[1], sy = (double)s[2], sz = (double)s[3];
  double a00 = (double)s[4] - (sx * sx) / cnt, a01 = (double)s[5] - (sx * sy) / cnt, a02 = (double)s[6] - (sx * sz) / cnt;
  double a11 = (double)s[7] - (sy * sy) / cnt, a12 = (double)s[8] - (sy * sz) / cnt, a22 = (double)s[9] - (sz * sz) / cnt;
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
  for (int sweep = 0; sweep < kNormalSweeps; ++sweep) {
    normal_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (0, 1), r = 2
    normal_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0, 2), r = 1
    normal_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1, 2), r = 0
  }
  // the smallest eigenvalue, ties to the lowest index, and the middle one.  The column is picked by ternaries: as an
  // `if` chain the device compiler parked V in scratch and indexed it (make resource-usage must show none)
  const bool take1 = a11 < a00;
  const double e01 = take1 ? a11 : a00;
  const bool take2 = a22 < e01;
  double x = take2 ? v02 : (take1 ? v01 : v00);
  double y = take2 ? v12 : (take1 ? v11 : v10);
  double z = take2 ? v22 : (take1 ? v21 : v20);
  const double lo01 = a00 < a11 ? a00 : a11, hi01 = a00 < a11 ? a11 : a00;
  const double t = hi01 < a22 ? hi01 : a22;
  const double mid = lo01 < t ? t : lo01;
  if (!(mid > 0.0)) return false;
  const double len = __builtin_sqrt((x * x + y * y) + z * z);
  x = x / len; y = y / len; z = z / len;
  // the component of largest magnitude positive, a tie to the lowest axis
  const double ax = x < 0.0 ? -x : x, ay = y < 0.0 ? -y : y, az = z < 0.0 ? -z : z;
  double lead = x, am = ax;
  if (ay > am) { lead = y; am = ay; }
  if (az > am) { lead = z; am = az; }
  if (lead < 0.0) { x = -x; y = -y; z = -z; }
  n[0] = (float)x; n[1] = (float)y; n[2] = (float)z;
  return true;
}

// "no normal": the three components are zeros (of either sign)
DPE_CHD bool normal_none(float x, float y, float z) {
  return ((depth_bits(x) | depth_bits(y) | depth_bits(z)) & 0x7FFFFFFFu) == 0u;
}

// the world normal n of the scan point (x, y, z) as the view `cam` sees it: turned towards the camera
DPE_CHD void normal_orient(const DpeCamera& cam, float x, float y, float z, const float n[3], float out[3]) {
  const float tx = cam.R[0] * x + cam.R[1] * y + cam.R[2] * z + cam.t[0];   // fz_project's (tx, ty, tz)
  const float ty = cam.R[3] * x + cam.R[4] * y + cam.R[5] * z + cam.t[1];
  const float tz = cam.R[6] * x + cam.R[7] * y + cam.R[8] * z + cam.t[2];
  const float cx = cam.R[0] * n[0] + cam.R[1] * n[1] + cam.R[2] * n[2];     // TransformNormal2RefCam's order
  const float cy = cam.R[3] * n[0] + cam.R[4] * n[1] + cam.R[5] * n[2];
  const float cz = cam.R[6] * n[0] + cam.R[7] * n[1] + cam.R[8] * n[2];
  const float s = (cx * tx + cy * ty) + cz * tz;
  const bool flip = s > 0.0f;
  out[0] = flip ? -n[0] : n[0];
  out[1] = flip ? -n[1] : n[1];
  out[2] = flip ? -n[2] : n[2];
}

// THE bin edges: E[b] = (float)cos(b degrees), b = 0..179 (E[0] = 1 is no edge).  Host only; the device gets the table
inline void normal_edges(float* E) {
  for (int b = 0; b < kNormalBins; ++b) E[b] = (float)std::cos((double)b * 3.14159265358979323846 / 180.0);
}
// a threshold in degrees as the cosine the score takes
inline float normal_cos_of_deg(double deg) { return (float)std::cos(deg * 3.14159265358979323846 / 180.0); }

// bin = #{ b in 1..179 : c < E[b] }; E falls strictly, so that is the largest such b (0 without one)
DPE_CHD int normal_bin(const float* E, float c) {
  int lo = 0, hi = kNormalBins - 1;   // c < E[b] holds for every b in 1..lo and for none above hi
  while (lo < hi) {
    const int m = (lo + hi + 1) >> 1;
    if (c < E[m]) lo = m; else hi = m - 1;
  }
  return lo;
}

// what one pixel of (est, gt) contributes
struct NormalPixel {
  bool gt_ok, est_ok, both;
  float c;   // the clamped cosine; meaningful where `both`
};

DPE_CHD NormalPixel normal_pixel(float ex, float ey, float ez, float gx, float gy, float gz) {
  NormalPixel p;
  const float ee = (ex * ex + ey * ey) + ez * ez, gg = (gx * gx + gy * gy) + gz * gz;
  p.est_ok = cloud_finite3(ex, ey, ez) && depth_ok(ee);
  p.gt_ok = cloud_finite3(gx, gy, gz) && depth_ok(gg);
  const float den = ee * gg;
  p.both = p.est_ok && p.gt_ok && depth_ok(den);
  const float c = ((ex * gx + ey * gy) + ez * gz) / __builtin_sqrtf(den);
  p.c = c < -1.0f ? -1.0f : (c > 1.0f ? 1.0f : c);
  return p;
}

// the two terms of the sums: +0.0 for a pixel that is not `both`, and never -0.0 (c <= 1)
DPE_CHD void normal_terms(const NormalPixel& p, double* t) {
  const double d = 1.0 - (double)p.c;
  t[0] = p.both ? d : 0.0;
  t[1] = p.both ? d * d : 0.0;
}

DPE_CHD float normal_error_code(const NormalPixel& p) { return p.both ? p.c : (p.gt_ok ? -2.0f : -3.0f); }

// the thresholds of one score as the kernel takes them: cosines
struct NormalTaus {
  float c[DPE_NORMAL_MAX_TAU];
  int n;
};

// The normal metric as the generic score sees it (k_map_score, host/map_eval.h): three floats per pixel, two sums and
// the histogram of kNormalBins bins over the edge table E.  The counters are DepthMetric's, then the bins
struct NormalMetric {
  static constexpr int kChannels = 3, kTerms = kNormalTerms, kMaxTau = DPE_NORMAL_MAX_TAU, kBins = kNormalBins;
  static constexpr int kCounters = 3 + kMaxTau + kBins;
  using Pixel = NormalPixel;
  using Taus = NormalTaus;
  using Score = DpeNormalScore;
  static DPE_CHD Pixel pixel(const float* est, const float* gt) { return normal_pixel(est[0], est[1], est[2], gt[0], gt[1], gt[2]); }
  static DPE_CHD bool hit(const Pixel& p, const float*, const Taus& T, int k) { return p.both && p.c > T.c[k]; }
  static DPE_CHD void terms(const Pixel& p, double* t) { normal_terms(p, t); }
  static DPE_CHD float error_code(const Pixel& p) { return normal_error_code(p); }
  static void edges(float* E) { normal_edges(E); }
  static DPE_CHD int bin(const float* E, const Pixel& p) { return normal_bin(E, p.c); }
  static void store(Score& s, const unsigned long long* counts, const double* sums) {
    for (int b = 0; b < kBins; ++b) s.hist[b] = (long long)counts[3 + kMaxTau + b];
    s.sum_dist = sums[0];
    s.sum_dist_sq = sums[1];
  }
  static void add(Score& total, const Score& s) {
    for (int b = 0; b < kBins; ++b) total.hist[b] += s.hist[b];
    total.sum_dist = total.sum_dist + s.sum_dist;
    total.sum_dist_sq = total.sum_dist_sq + s.sum_dist_sq;
  }
};

}  // namespace dpe
