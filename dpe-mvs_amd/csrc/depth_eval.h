// depth_eval.h — the arithmetic of the depth-map evaluation (dpe_cloud_render_view and dpe_depth_score of
// include/dpe_mvs.h, which states the contract) that the host (host/depth_eval.cpp) shares with the kernels
// (pass_render.h): the projection of a scan point and its centre pixel (fusion_world.h's), the z-buffer's word, the test for a usable depth
// and what one pixel contributes to a score, gathered in DepthMetric for the code that scores any map
// (k_map_score, host/map_eval.h).  Plain C++, -ffp-contract=off like everything here: every operation below is one
// rounded single-precision operation with IEEE division, unless a double is written.
#pragma once
#include "../../include/dpe_mvs.h"
#include "cloud_dist.h"     // cloud_finite3
#include "fusion_world.h"   // fz_project, fz_pixel

#include <cstring>

namespace dpe {

constexpr int kDepthMaxSplat = 8;
constexpr int kDepthTerms = 3;                  // e, rel, e * e
constexpr uint32_t kDepthEmpty = 0x7F800000u;   // +inf: a pixel of the z-buffer that no point covers yet

DPE_CHD uint32_t depth_bits(float v) {
  union { float f; uint32_t u; } b;
  b.f = v;
  return b.u;
}

// a usable depth: positive and finite, decided on the bit pattern (a NaN, a zero of either sign and every
// negative number fail; positive finite floats order as these integers)
DPE_CHD bool depth_ok(float v) {
  const uint32_t u = depth_bits(v);
  return u > 0u && u < kDepthEmpty;
}

// One scan point in a view: false when it renders nothing, else its centre pixel and the bits of its depth
DPE_CHD bool depth_point(const DpeCamera& cam, float x, float y, float z, int& cx, int& cy, uint32_t& zbits) {
  if (!cloud_finite3(x, y, z)) return false;
  float px, py, d;
  fz_project(FP3{x, y, z}, cam, px, py, d);
  if (!depth_ok(d)) return false;
  zbits = depth_bits(d);
  return fz_pixel(px, py, cam.width, cam.height, cx, cy);   // the centre pixel by fusion's rule
}

// The word of a render's z-buffer and its empty value.  uint32_t: the bits of the depth.  unsigned long long: the
// render with winners, bits(z) << 32 | point index, whose minimum is the lexicographic minimum of (bits(z), index)
template <typename Word>
struct RenderWord;
template <>
struct RenderWord<uint32_t> {
  static constexpr uint32_t kEmpty = kDepthEmpty;
  static DPE_CHD uint32_t make(uint32_t zbits, uint32_t) { return zbits; }
};
template <>
struct RenderWord<unsigned long long> {
  static constexpr unsigned long long kEmpty = ((unsigned long long)kDepthEmpty << 32) | 0xFFFFFFFFull;
  static DPE_CHD unsigned long long make(uint32_t zbits, uint32_t index) { return ((unsigned long long)zbits << 32) | index; }
};

// what one pixel of (est, gt) contributes
struct DepthPixel {
  bool gt_ok, est_ok, both;
  float e, rel;   // |est - gt| and e / gt; meaningful where `both`
};

DPE_CHD DepthPixel depth_pixel(float est, float gt) {
  DepthPixel p;
  p.gt_ok = depth_ok(gt);
  p.est_ok = depth_ok(est);
  p.both = p.gt_ok && p.est_ok;
  p.e = __builtin_fabsf(est - gt);
  p.rel = p.e / gt;
  return p;
}

DPE_CHD bool depth_hit(const DepthPixel& p, float gt, float tau, int mode) {
  return p.both && (mode == DPE_DEPTH_TAU_ABS ? p.e < tau : p.e < tau * gt);
}

// the three terms of the sums: +0.0 for a pixel that is not `both`, and never -0.0 (e and rel are >= +0.0)
DPE_CHD void depth_terms(const DepthPixel& p, double* t) {
  t[0] = p.both ? (double)p.e : 0.0;
  t[1] = p.both ? (double)p.rel : 0.0;
  t[2] = p.both ? (double)p.e * (double)p.e : 0.0;
}

DPE_CHD float depth_error_code(const DepthPixel& p) { return p.both ? p.e : (p.gt_ok ? -1.0f : -2.0f); }

// the thresholds of one score as the kernel takes them
struct DepthTaus {
  float tau[DPE_DEPTH_MAX_TAU];
  int n, mode;
};

// The depth metric as the generic score sees it (k_map_score, host/map_eval.h): one float per pixel, three sums, no
// histogram.  The counters are n_gt, n_est, n_both, within[kMaxTau], then the kBins bins
struct DepthMetric {
  static constexpr int kChannels = 1, kTerms = kDepthTerms, kMaxTau = DPE_DEPTH_MAX_TAU, kBins = 0;
  static constexpr int kCounters = 3 + kMaxTau + kBins;
  using Pixel = DepthPixel;
  using Taus = DepthTaus;
  using Score = DpeDepthScore;
  static DPE_CHD Pixel pixel(const float* est, const float* gt) { return depth_pixel(est[0], gt[0]); }
  static DPE_CHD bool hit(const Pixel& p, const float* gt, const Taus& T, int k) { return depth_hit(p, gt[0], T.tau[k], T.mode); }
  static DPE_CHD void terms(const Pixel& p, double* t) { depth_terms(p, t); }
  static DPE_CHD float error_code(const Pixel& p) { return depth_error_code(p); }
  static void store(Score& s, const unsigned long long*, const double* sums) {
    s.sum_abs = sums[0];
    s.sum_rel = sums[1];
    s.sum_sq = sums[2];
  }
  static void add(Score& total, const Score& s) {
    total.sum_abs = total.sum_abs + s.sum_abs;
    total.sum_rel = total.sum_rel + s.sum_rel;
    total.sum_sq = total.sum_sq + s.sum_sq;
  }
};

// the score of npx pixels from a metric's counters and sums, on either path; every other byte zero (the structs are
// compared as bytes)
template <typename M>
typename M::Score score_of(size_t npx, int n_tau, const unsigned long long* counts, const double* sums) {
  typename M::Score s;
  memset(&s, 0, sizeof s);
  s.n_px = (long long)npx;
  s.n_gt = (long long)counts[0];
  s.n_est = (long long)counts[1];
  s.n_both = (long long)counts[2];
  for (int k = 0; k < n_tau; ++k) s.within[k] = (long long)counts[3 + k];
  M::store(s, counts, sums);
  return s;
}

}  // namespace dpe
