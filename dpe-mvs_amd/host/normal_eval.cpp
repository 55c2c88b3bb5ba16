// normal_eval.cpp — the normal-map evaluation on the host: the normals of a scan's points by PCA over the hashed grid,
// the render of the winning point's normal into one view and the score of one normal map as include/dpe_mvs.h states
// them (dpe_cloud_normals, dpe_cloud_render_view_normals, dpe_normal_score), with the pairwise tree taken literally,
// what is derived from a score, and the evaluation of a dense folder over either path.  The loops, map_eval.h's over
// NormalMetric beside the point normals' own, are the yardstick of the kernels (csrc/pass_normals.h, csrc/pass_render.h)
// and what runs without a GPU; the arithmetic is csrc/normal_eval.h's, which the
// kernels share.  No counterpart in the reference.
#include "map_eval.h"
#include "cloud_index.h"
#include "../csrc/normal_eval.h"

#include <atomic>
#include <climits>
#include <cmath>

namespace dpe_host {

namespace {

using dpe::kNormalBins;
using dpe::kNormalSums;
using dpe::NormalMetric;

// points [i0, i1) of the cloud the index was built from: k_cloud_normal's walk, the same no-double-count rule
void normals_range(const CloudIndex& ix, const float* xyz, size_t i0, size_t i1, double S, int min_nb, float* normal,
                   int32_t* count, long long* sums) {
  const dpe::CloudGrid& g = ix.g;
  for (size_t i = i0; i < i1; ++i) {
    const float qx = xyz[3 * i], qy = xyz[3 * i + 1], qz = xyz[3 * i + 2];
    long long s[kNormalSums] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (dpe::cloud_finite3(qx, qy, qz)) {
      const dpe::NormalWalk w = dpe::normal_walk(g, qx, qy, qz);
      for (int k = 0; k < 27; ++k) {
        int32_t cx, cy, cz;
        if (!dpe::normal_cell(w, k, cx, cy, cz)) continue;
        const uint32_t b = dpe::cloud_bucket(cx, cy, cz, g.mask);
        if (dpe::normal_bucket_seen(w, g.mask, k, b)) continue;
        const int j1 = ix.end[b];
        for (int j = b ? ix.end[b - 1] : 0; j < j1; ++j) {
          const float* t = ix.st.data() + 3 * (size_t)j;
          if (dpe::cloud_d2(qx, qy, qz, t[0], t[1], t[2]) < ix.r2) dpe::normal_add(qx, qy, qz, t[0], t[1], t[2], S, s);
        }
      }
    }
    dpe::normal_solve(s, (long long)min_nb, normal + 3 * i);
    count[i] = (int32_t)s[0];
    if (sums) std::memcpy(sums + (size_t)kNormalSums * i, s, sizeof s);
  }
}

bool score_args_ok(const float* cos_tau, int n_tau, std::string& err) {
  if (!cos_tau || n_tau < 1 || n_tau > DPE_NORMAL_MAX_TAU) { err = "normal_score: 1 to 16 thresholds expected"; return false; }
  for (int k = 0; k < n_tau; ++k)
    if (!std::isfinite(cos_tau[k]) || !(cos_tau[k] >= -1.0f && cos_tau[k] <= 1.0f)) {
      err = "normal_score: a threshold's cosine is not in [-1, 1]";
      return false;
    }
  return true;
}

bool normals_args_ok(const float* xyz, size_t n, float radius, int min_nb, std::string& err) {
  if (n > (size_t)INT_MAX || (!xyz && n)) { err = "cloud_normals: bad argument"; return false; }
  if (!cloud_radius_ok(radius)) { err = "cloud_normals: the radius is not a finite positive number"; return false; }
  if (min_nb < dpe::kNormalMinNb) { err = "cloud_normals: at least 3 neighbours must be asked for"; return false; }
  return true;
}

bool render_args_ok(const float* xyz, const float* normals, size_t n, const DpeCamera* cam, int splat, std::string& err) {
  if (n > (size_t)INT_MAX || ((!xyz || !normals) && n) || !cam) { err = "cloud_render_normals: bad argument"; return false; }
  if (cam->width < 1 || cam->height < 1) { err = "cloud_render_normals: the camera's width and height must be at least 1"; return false; }
  if (splat < 0 || splat > DPE_DEPTH_MAX_SPLAT) { err = "cloud_render_normals: the splat half-width must be 0 to 8"; return false; }
  return true;
}

}  // namespace

bool cloud_normals(const float* xyz, size_t n, float radius, int min_nb, float* normal, int32_t* count, long long* sums,
                   std::string& err) {
  if (!normals_args_ok(xyz, n, radius, min_nb, err)) return false;
  if (n == 0) return true;
  if (!normal || !count) { err = "cloud_normals: bad argument"; return false; }
  CloudIndex ix;
  if (!ix.build(xyz, n, radius, "cloud_normals", err)) return false;
  if (ix.finite == 0) {
    std::memset(normal, 0, 3 * n * sizeof(float));
    std::memset(count, 0, n * sizeof(int32_t));
    if (sums) std::memset(sums, 0, (size_t)kNormalSums * n * sizeof(long long));
    return true;
  }
  const double S = dpe::normal_scale(radius);
  const size_t kChunk = 1024;
  const size_t chunks = (n + kChunk - 1) / kChunk;
  std::atomic<size_t> next{0};
  run_on_threads((int)std::min<size_t>((size_t)host_threads(), chunks), [&](int) {
    for (size_t ch = next++; ch < chunks; ch = next++)
      normals_range(ix, xyz, ch * kChunk, std::min(n, (ch + 1) * kChunk), S, min_nb, normal, count, sums);
  });
  return true;
}

bool cloud_render_normals(const float* xyz, const float* normals, size_t n, const DpeCamera& cam, int splat, float* depth,
                          float* normal, std::string& err) {
  if (!render_args_ok(xyz, normals, n, &cam, splat, err)) return false;
  const std::vector<unsigned long long> zb = render_zbuffer<unsigned long long>(xyz, n, cam, splat);
  for (size_t p = 0; p < zb.size(); ++p) {
    const unsigned long long word = zb[p];
    uint32_t z = (uint32_t)(word >> 32);
    const bool empty = z == dpe::kDepthEmpty;
    if (empty) z = 0u;
    if (depth) std::memcpy(depth + p, &z, sizeof z);
    if (!normal) continue;
    float o[3] = {0.0f, 0.0f, 0.0f};
    if (!empty) {
      const size_t at = 3 * (size_t)(uint32_t)word;
      if (!dpe::normal_none(normals[at], normals[at + 1], normals[at + 2]))
        dpe::normal_orient(cam, xyz[at], xyz[at + 1], xyz[at + 2], normals + at, o);
    }
    std::memcpy(normal + 3 * p, o, sizeof o);
  }
  return true;
}

bool normal_score(const float* est, const float* gt, int w, int h, const float* cos_tau, int n_tau, DpeNormalScore* out,
                  float* errmap, std::string& err) {
  if (!est || !gt || w < 1 || h < 1 || !out) { err = "normal_score: bad argument"; return false; }
  if (!score_args_ok(cos_tau, n_tau, err)) return false;
  dpe::NormalTaus T{};
  std::copy(cos_tau, cos_tau + n_tau, T.c);
  T.n = n_tau;
  map_score<NormalMetric>(est, gt, w, h, T, out, errmap);
  return true;
}

void normal_stats(const DpeNormalScore& s, int n_tau, DpeNormalStats* out) {
  std::memset(out, 0, sizeof *out);
  stats_shares<NormalMetric>(s, n_tau, out->share, out->completeness);
  if (!s.n_both) return;
  const double nb = (double)s.n_both;
  out->mean_cos_dist = s.sum_dist / nb;
  // from the histogram: a pixel of bin b stands at b + 0.5 degrees
  double weighted = 0.0;
  long long run = 0;
  bool have_median = false;
  for (int b = 0; b < kNormalBins; ++b) {
    weighted = weighted + (double)s.hist[b] * ((double)b + 0.5);
    run += s.hist[b];
    if (!have_median && 2 * run >= s.n_both) { out->median_deg = (double)b + 0.5; have_median = true; }
  }
  out->mean_deg = weighted / nb;
}

namespace {

// map_eval's hooks; the scan's normals are estimated once per folder
struct NormalEval {
  using Metric = NormalMetric;
  using Options = DpeNormalEvalOptions;
  using Image = DpeNormalImage;
  static constexpr const char *kWho = "normal_eval", *kMap = "normal.npy", *kGtName = "normal_gt.npy", *kErrName = "normal_error.npy";
  std::vector<float> gt_normals;
  static bool read(const std::string& path, std::vector<float>& data, int& w, int& h, std::string& err) {
    return read_npy_f32x3(path, data, w, h, err);
  }
  bool args_ok(const Options& o, const float* xyz, size_t n, bool from_maps, std::string& err) {
    if (!score_args_ok(o.cos_tau, o.n_tau, err)) return false;
    if (from_maps) return true;
    if (!normals_args_ok(xyz, n, o.radius, o.min_nb, err)) return false;
    if (o.splat < 0 || o.splat > DPE_DEPTH_MAX_SPLAT) { err = "cloud_render_normals: the splat half-width must be 0 to 8"; return false; }
    return true;
  }
  bool prepare(DpeContext* ctx, const Options& o, const float* xyz, size_t n, std::string& err) {
    gt_normals.resize(3 * n);
    std::vector<int32_t> counts(n);
    if (!ctx) return cloud_normals(xyz, n, o.radius, o.min_nb, gt_normals.data(), counts.data(), nullptr, err);
    return dpe_cloud_normals(ctx, xyz, n, o.radius, o.min_nb, gt_normals.data(), counts.data(), nullptr) == 0 &&
           dpe_cloud_render_stage_normals(ctx, xyz, gt_normals.data(), n) == 0;
  }
  int render_device(DpeContext* ctx, const DpeCamera& cam, const Options& o, float* gt) {
    return dpe_cloud_render_view_normals(ctx, &cam, o.splat, nullptr, gt);
  }
  bool render_host(const float* xyz, size_t n, const DpeCamera& cam, const Options& o, float* gt, std::string& err) {
    return cloud_render_normals(xyz, gt_normals.data(), n, cam, o.splat, nullptr, gt, err);
  }
  int score_device(DpeContext* ctx, const float* est, const float* gt, int w, int h, const Options& o, DpeNormalScore* out, float* em) {
    return dpe_normal_score(ctx, est, gt, w, h, o.cos_tau, o.n_tau, out, em);
  }
  bool score_host(const float* est, const float* gt, int w, int h, const Options& o, DpeNormalScore* out, float* em, std::string& err) {
    return normal_score(est, gt, w, h, o.cos_tau, o.n_tau, out, em, err);
  }
};

}  // namespace

}  // namespace dpe_host

extern "C" {

int dpe_host_cloud_normals(const float* xyz, size_t n, float radius, int min_nb, float* normal_out, int32_t* count_out,
                           long long* sums_out) {
  return dpe_host::c_entry(
      [&](std::string& err) { return dpe_host::cloud_normals(xyz, n, radius, min_nb, normal_out, count_out, sums_out, err); });
}

int dpe_host_cloud_render_normals(const float* xyz, const float* normals, size_t n, const DpeCamera* cam, int splat,
                                  float* depth_out, float* normal_out) {
  return dpe_host::c_entry(
      [&](std::string& err) { return cam && dpe_host::cloud_render_normals(xyz, normals, n, *cam, splat, depth_out, normal_out, err); },
      "cloud_render_normals: bad argument");
}

int dpe_host_normal_score(const float* est, const float* gt, int w, int h, const float* cos_tau, int n_tau, DpeNormalScore* out,
                          float* err_or_null) {
  return dpe_host::c_entry(
      [&](std::string& err) { return dpe_host::normal_score(est, gt, w, h, cos_tau, n_tau, out, err_or_null, err); });
}

void dpe_host_normal_edges(float* edges) {
  if (edges) dpe::normal_edges(edges);
}

float dpe_host_normal_cos(double deg) { return dpe::normal_cos_of_deg(deg); }

void dpe_host_normal_stats(const DpeNormalScore* s, int n_tau, DpeNormalStats* out) {
  if (s && out) dpe_host::normal_stats(*s, n_tau, out);
}

int dpe_host_read_npy_f32x3(const char* path, float* data, size_t cap, int* w, int* h) {
  return dpe_host::read_npy_entry(dpe_host::read_npy_f32x3, path, data, cap, w, h);
}

int dpe_host_normal_eval(const DpeNormalEvalOptions* opt, const float* gt_xyz, size_t n_gt, DpeNormalImage* rows, size_t cap,
                         size_t* n_rows, DpeNormalScore* total) {
  dpe_host::NormalEval hooks;
  return dpe_host::c_entry([&](std::string& err) { return opt && dpe_host::map_eval(hooks, *opt, gt_xyz, n_gt, rows, cap, n_rows, total, err); },
                           "normal_eval: bad argument");
}

}  // extern "C"
