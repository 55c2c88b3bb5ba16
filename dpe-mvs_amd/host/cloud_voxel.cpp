// cloud_voxel.cpp — voxel down-sampling and cropping of point clouds on the host, and the evaluation with that
// preparation: dpe_host_cloud_voxel is the contract of dpe_cloud_voxel (include/dpe_mvs.h) as a serial loop with
// a hash map over the header functions the kernels use (csrc/cloud_dist.h), so both paths give equal bits; it is
// the yardstick of the device path and what runs without a GPU.  No counterpart in the reference.
#include "host.h"

#include "../csrc/cloud_dist.h"

#include <climits>
#include <cmath>
#include <string>
#include <unordered_map>
#include <vector>

namespace dpe_host {

namespace {

struct Cell {
  int32_t x, y, z;
  bool operator==(const Cell& o) const { return x == o.x && y == o.y && z == o.z; }
};
struct CellHash {
  size_t operator()(const Cell& c) const {
    uint64_t h = (uint64_t)(uint32_t)c.x * 0x9E3779B97F4A7C15ull;
    h = (h ^ (uint64_t)(uint32_t)c.y) * 0xC2B2AE3D27D4EB4Full;
    h = (h ^ (uint64_t)(uint32_t)c.z) * 0x165667B19E3779F9ull;
    return (size_t)(h ^ (h >> 29));
  }
};

// a voxel's record before the division: records are created in the order the loop meets the voxels, which is
// ascending `first`
struct Acc {
  Cell c;
  int32_t first, count;
  unsigned long long sum[3], csum[3];
};

}  // namespace

bool cloud_voxel(const float* xyz, size_t n, const uint8_t* rgb, float voxel, float* out_xyz, uint8_t* out_rgb,
                 int32_t* out_first, int32_t* out_count, size_t cap, size_t* k, std::string& err) {
  if (n > (size_t)INT_MAX || (!xyz && n) || !k || !(std::isfinite(voxel) && voxel > 0.0f) ||
      (cap != 0 && (!out_xyz || !out_first || !out_count || (rgb && !out_rgb)))) {
    err = "cloud_voxel: bad argument";
    return false;
  }
  *k = 0;
  float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  size_t finite = 0;
  for (size_t i = 0; i < n; ++i) {
    const float* p = xyz + 3 * i;
    if (!dpe::cloud_finite3(p[0], p[1], p[2])) continue;
    for (int a = 0; a < 3; ++a) {
      if (!finite || p[a] < lo[a]) lo[a] = p[a];
      if (!finite || p[a] > hi[a]) hi[a] = p[a];
    }
    ++finite;
  }
  if (finite == 0) return true;
  dpe::VoxelGrid g;
  if (!dpe::voxel_grid_make(lo, hi, voxel, &g)) {
    err = "cloud_voxel: voxel too small for the cloud's extent";
    return false;
  }
  std::unordered_map<Cell, size_t, CellHash> at;
  std::vector<Acc> acc;
  for (size_t i = 0; i < n; ++i) {
    const float* p = xyz + 3 * i;
    if (!dpe::cloud_finite3(p[0], p[1], p[2])) continue;
    Cell c;
    const uint32_t q[3] = {dpe::voxel_cell_frac(p[0], g.o[0], g.h, &c.x), dpe::voxel_cell_frac(p[1], g.o[1], g.h, &c.y),
                           dpe::voxel_cell_frac(p[2], g.o[2], g.h, &c.z)};
    const auto it = at.emplace(c, acc.size());
    if (it.second) acc.push_back(Acc{c, (int32_t)i, 0, {0, 0, 0}, {0, 0, 0}});
    Acc& r = acc[it.first->second];
    ++r.count;
    for (int a = 0; a < 3; ++a) {
      r.sum[a] += q[a];
      if (rgb) r.csum[a] += rgb[3 * i + a];
    }
  }
  *k = acc.size();
  if (acc.size() > cap) {
    err = "cloud_voxel: output buffers too small for the voxels";
    return false;
  }
  for (size_t r = 0; r < acc.size(); ++r) {
    const Acc& v = acc[r];
    const int32_t c[3] = {v.c.x, v.c.y, v.c.z};
    for (int a = 0; a < 3; ++a) {
      out_xyz[3 * r + a] = dpe::voxel_coord(g.o[a], g.h, c[a], v.sum[a], v.count);
      if (rgb) out_rgb[3 * r + a] = dpe::voxel_colour(v.csum[a], v.count);
    }
    out_first[r] = v.first;
    out_count[r] = v.count;
  }
  return true;
}

void cloud_crop(const float* xyz, size_t n, const float lo[3], const float hi[3], std::vector<int32_t>& keep) {
  keep.clear();
  for (size_t i = 0; i < n; ++i) {
    const float* p = xyz + 3 * i;
    if (!dpe::cloud_finite3(p[0], p[1], p[2])) continue;
    bool in = true;
    for (int a = 0; a < 3; ++a) in = in && lo[a] <= p[a] && p[a] <= hi[a];
    if (in) keep.push_back((int32_t)i);
  }
}

// one cloud through the preparation: `pts` becomes what is scored
bool cloud_prepare(DpeContext* ctx, const float* xyz, size_t n, const DpeCloudPrep& prep, bool crop, std::vector<float>& pts,
                   std::string& err) {
  pts.assign(xyz, xyz + 3 * n);
  if (crop) {
    std::vector<int32_t> keep;
    cloud_crop(xyz, n, prep.crop_lo, prep.crop_hi, keep);
    pts.resize(3 * keep.size());
    for (size_t r = 0; r < keep.size(); ++r)
      for (int a = 0; a < 3; ++a) pts[3 * r + a] = xyz[3 * (size_t)keep[r] + a];
  }
  if (prep.voxel == 0.0f) return true;
  const size_t m = pts.size() / 3;
  std::vector<float> out(3 * m + 3);
  std::vector<int32_t> first(m + 1), count(m + 1);
  size_t k = 0;
  if (!ctx) {
    if (!cloud_voxel(pts.data(), m, nullptr, prep.voxel, out.data(), nullptr, first.data(), count.data(), m, &k, err)) return false;
  } else if (dpe_cloud_voxel(ctx, pts.data(), m, nullptr, prep.voxel, out.data(), nullptr, first.data(), count.data(), m, &k) != 0) {
    err = device_error("cloud_voxel", "dpe_cloud_voxel");
    return false;
  }
  out.resize(3 * k);
  pts.swap(out);
  return true;
}

bool cloud_prep_args(const float* recon, size_t n, const float* gt, size_t m, const DpeCloudPrep& prep, std::string& err) {
  if (n > (size_t)INT_MAX || m > (size_t)INT_MAX || (!recon && n) || (!gt && m)) { err = "cloud_eval: bad cloud"; return false; }
  if (!(prep.voxel == 0.0f || (std::isfinite(prep.voxel) && prep.voxel > 0.0f))) {
    err = "cloud_eval: the voxel edge is not a finite positive number";
    return false;
  }
  if (prep.use_crop) {
    for (int a = 0; a < 3; ++a)
      if (!(prep.crop_lo[a] <= prep.crop_hi[a])) { err = "cloud_eval: the crop box is empty or not a number"; return false; }
  }
  return true;
}

bool cloud_eval_prep_in(DpeContext* ctx, const float* recon, size_t n, const float* gt, size_t m, const float* tau, int n_tau,
                        float radius, DpeCloudPrep* prep, DpeCloudEval* out, std::string& err) {
  prep->n_recon_in = n;
  prep->n_gt_in = m;
  std::vector<float> a, b;
  return cloud_prepare(ctx, recon, n, *prep, prep->use_crop != 0, a, err) && cloud_prepare(ctx, gt, m, *prep, prep->use_crop != 0, b, err) &&
         cloud_eval_in(ctx, a.data(), a.size() / 3, b.data(), b.size() / 3, tau, n_tau, radius, out, err);
}

bool cloud_eval_prep(const float* recon, size_t n, const float* gt, size_t m, const float* tau, int n_tau, float radius,
                     int gpu_index, DpeCloudPrep* prep, DpeCloudEval* out, std::string& err) {
  if (!prep) return cloud_eval(recon, n, gt, m, tau, n_tau, radius, gpu_index, out, err);
  if (!cloud_prep_args(recon, n, gt, m, *prep, err)) return false;
  OwnedContext own(gpu_index, "cloud_eval", err);
  return own.ok && cloud_eval_prep_in(own.ctx, recon, n, gt, m, tau, n_tau, radius, prep, out, err);
}

}  // namespace dpe_host

extern "C" {

int dpe_host_cloud_voxel(const float* xyz, size_t n, const uint8_t* rgb, float voxel, float* out_xyz, uint8_t* out_rgb,
                         int32_t* out_first, int32_t* out_count, size_t cap, size_t* k) {
  return dpe_host::c_entry(
      [&](std::string& err) { return dpe_host::cloud_voxel(xyz, n, rgb, voxel, out_xyz, out_rgb, out_first, out_count, cap, k, err); });
}

size_t dpe_host_cloud_crop(const float* xyz, size_t n, const uint8_t* rgb, const float* lo, const float* hi, float* out_xyz,
                           uint8_t* out_rgb, int32_t* out_index) {
  if ((!xyz && n) || !lo || !hi || n > (size_t)INT_MAX) return 0;
  std::vector<int32_t> keep;
  dpe_host::cloud_crop(xyz, n, lo, hi, keep);
  for (size_t r = 0; r < keep.size(); ++r) {
    const size_t i = (size_t)keep[r];
    for (int a = 0; a < 3; ++a) {
      if (out_xyz) out_xyz[3 * r + a] = xyz[3 * i + a];
      if (out_rgb && rgb) out_rgb[3 * r + a] = rgb[3 * i + a];
    }
    if (out_index) out_index[r] = keep[r];
  }
  return keep.size();
}

int dpe_host_cloud_eval_prep(const float* recon, size_t n, const float* gt, size_t m, const float* tau, int n_tau, float radius,
                             int gpu_index, DpeCloudPrep* prep, DpeCloudEval* out) {
  return dpe_host::c_entry(
      [&](std::string& err) { return dpe_host::cloud_eval_prep(recon, n, gt, m, tau, n_tau, radius, gpu_index, prep, out, err); });
}

}  // extern "C"
