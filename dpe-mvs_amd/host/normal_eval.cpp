// normal_eval.cpp — the normal-map evaluation on the host: the normals of a scan's points by PCA over the hashed grid,
// the render of the winning point's normal into one view and the score of one normal map as include/dpe_mvs.h states
// them (dpe_cloud_normals, dpe_cloud_render_view_normals, dpe_normal_score), with the pairwise tree taken literally,
// what is derived from a score, and the evaluation of a dense folder over either path.  The loops are the yardstick of
// the kernels (csrc/pass_normals.h) and what runs without a GPU; the arithmetic is csrc/normal_eval.h's, which the
// kernels share.  No counterpart in the reference.
#include "host.h"
#include "cloud_index.h"
#include "pairwise_tree.h"
#include "parallel.h"
#include "../csrc/normal_eval.h"

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstring>
#include <filesystem>
#include <string>
#include <vector>

namespace fs = std::filesystem;

namespace dpe_host {

namespace {

using dpe::kNormalBins;
using dpe::kNormalSums;
using dpe::kNormalTerms;

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

// points [i0, i1) into the z-buffer of words bits(z) << 32 | index
void render_range(const float* xyz, size_t i0, size_t i1, const DpeCamera& cam, int s, unsigned long long* zb) {
  const int w = cam.width, h = cam.height;
  for (size_t i = i0; i < i1; ++i) {
    int cx, cy;
    uint32_t z;
    if (!dpe::depth_point(cam, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], cx, cy, z)) continue;
    const unsigned long long word = dpe::normal_word(z, (uint32_t)i);
    const int x0 = std::max(0, cx - s), x1 = std::min(w - 1, cx + s);
    const int y0 = std::max(0, cy - s), y1 = std::min(h - 1, cy + s);
    for (int y = y0; y <= y1; ++y) {
      unsigned long long* row = zb + (size_t)y * (size_t)w;
      for (int x = x0; x <= x1; ++x)
        if (word < row[x]) row[x] = word;
    }
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

constexpr size_t kRenderPerThread = 1u << 16;   // fewer points than this per thread are not worth a z-buffer

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
  const size_t npx = (size_t)cam.width * (size_t)cam.height;
  const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)host_threads(), n / kRenderPerThread));
  // one z-buffer of words per thread over its share of the points, merged by minimum below
  std::vector<unsigned long long> zb((size_t)nt * npx, dpe::kNormalEmptyWord);
  run_on_threads(nt, [&](int t) { render_range(xyz, n * t / nt, n * (t + 1) / nt, cam, splat, zb.data() + (size_t)t * npx); });
  for (size_t p = 0; p < npx; ++p) {
    unsigned long long word = zb[p];
    for (int t = 1; t < nt; ++t) word = std::min(word, zb[(size_t)t * npx + p]);
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
  DpeNormalScore s;
  std::memset(&s, 0, sizeof s);   // the structs are compared as bytes
  float E[kNormalBins];
  dpe::normal_edges(E);
  const size_t npx = (size_t)w * (size_t)h;
  PairwiseTree<kNormalTerms> tree;
  for (size_t i = 0; i < npx; ++i) {
    const float* e = est + 3 * i;
    const float* g = gt + 3 * i;
    const dpe::NormalPixel p = dpe::normal_pixel(e[0], e[1], e[2], g[0], g[1], g[2]);
    s.n_gt += p.gt_ok;
    s.n_est += p.est_ok;
    s.n_both += p.both;
    for (int k = 0; k < n_tau; ++k) s.within[k] += p.both && p.c > cos_tau[k];
    if (p.both) s.hist[dpe::normal_bin(E, p.c)] += 1;
    double t[kNormalTerms];
    dpe::normal_terms(p, t);
    tree.push(t);
    if (errmap) errmap[i] = dpe::normal_error_code(p);
  }
  double sums[kNormalTerms];
  tree.finish(sums);
  s.n_px = (long long)npx;
  s.sum_dist = sums[0];
  s.sum_dist_sq = sums[1];
  *out = s;
  return true;
}

void normal_stats(const DpeNormalScore& s, int n_tau, DpeNormalStats* out) {
  std::memset(out, 0, sizeof *out);
  const double nb = (double)s.n_both, ng = (double)s.n_gt;
  for (int k = 0; k < n_tau && k < DPE_NORMAL_MAX_TAU; ++k) {
    out->share[k] = s.n_both ? (double)s.within[k] / nb : 0.0;
    out->completeness[k] = s.n_gt ? (double)s.within[k] / ng : 0.0;
  }
  if (!s.n_both) return;
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

void normal_add(DpeNormalScore* total, const DpeNormalScore& s) {
  total->n_px += s.n_px;
  total->n_gt += s.n_gt;
  total->n_est += s.n_est;
  total->n_both += s.n_both;
  for (int k = 0; k < DPE_NORMAL_MAX_TAU; ++k) total->within[k] += s.within[k];
  for (int b = 0; b < kNormalBins; ++b) total->hist[b] += s.hist[b];
  total->sum_dist = total->sum_dist + s.sum_dist;
  total->sum_dist_sq = total->sum_dist_sq + s.sum_dist_sq;
}

namespace {

const char* map_name_of(const char* name) { return name && *name ? name : "normal.npy"; }

bool normal_eval(const DpeNormalEvalOptions& o, const float* gt_xyz, size_t n_gt, DpeNormalImage* rows, size_t cap, size_t* n_rows,
                 DpeNormalScore* total, std::string& err) {
  if (!o.dense_folder || !n_rows || !total || (!rows && cap)) { err = "normal_eval: bad argument"; return false; }
  if (!score_args_ok(o.cos_tau, o.n_tau, err)) return false;
  const bool from_maps = o.gt_maps_dir && *o.gt_maps_dir;
  if (!from_maps) {
    if (!normals_args_ok(gt_xyz, n_gt, o.radius, o.min_nb, err)) return false;
    if (o.splat < 0 || o.splat > DPE_DEPTH_MAX_SPLAT) { err = "cloud_render_normals: the splat half-width must be 0 to 8"; return false; }
  }
  const std::string dense = o.dense_folder, map = map_name_of(o.map_name);
  std::vector<int> ids;
  if (!eval_list("normal_eval", dense, map, ids, err)) return false;
  *n_rows = ids.size();
  if (cap < ids.size()) { err = "normal_eval: room for fewer rows than images"; return false; }
  OwnedContext own(o.gpu_index, "normal_eval", err);
  if (!own.ok) return false;
  DpeContext* ctx = own.ctx;
  auto device_failed = [&]() { err = std::string("normal_eval: ") + dpe_last_error(); return false; };
  // the scan's normals, once, and the staging of scan and normals
  std::vector<float> gt_normals;
  if (!from_maps) {
    gt_normals.resize(3 * n_gt);
    std::vector<int32_t> counts(n_gt);
    if (ctx) {
      if (dpe_cloud_normals(ctx, gt_xyz, n_gt, o.radius, o.min_nb, gt_normals.data(), counts.data(), nullptr) != 0) return device_failed();
      if (dpe_cloud_render_stage_normals(ctx, gt_xyz, gt_normals.data(), n_gt) != 0) return device_failed();
    } else if (!cloud_normals(gt_xyz, n_gt, o.radius, o.min_nb, gt_normals.data(), counts.data(), nullptr, err)) {
      return false;
    }
  }
  DpeNormalScore sum;
  std::memset(&sum, 0, sizeof sum);
  std::vector<float> est, gt, errmap;
  std::vector<DpeNormalImage> done(ids.size());   // a failure leaves the caller's rows alone
  for (size_t i = 0; i < ids.size(); ++i) {
    const fs::path rf = fs::path(dense) / "DPE" / fmt_index(ids[i]);
    int w = 0, h = 0;
    if (!read_npy_f32x3((rf / map).string(), est, w, h, err)) return false;
    const size_t npx = (size_t)w * (size_t)h;
    const bool want_gt = !ctx || from_maps || o.write_maps;   // the ground truth on the host
    if (want_gt) gt.resize(3 * npx);
    if (o.write_maps) errmap.resize(npx);
    if (from_maps) {
      int gw = 0, gh = 0;
      const std::string path = (fs::path(o.gt_maps_dir) / (fmt_index(ids[i]) + ".npy")).string();
      if (!read_npy_f32x3(path, gt, gw, gh, err)) return false;
      if (gw != w || gh != h) { err = "normal_eval: size mismatch: " + path + " is not of the size of " + (rf / map).string(); return false; }
    } else {
      DpeCamera cam;
      if (!map_camera(dense, ids[i], w, h, cam, err)) return false;
      if (ctx) {
        if (dpe_cloud_render_view_normals(ctx, &cam, o.splat, nullptr, want_gt ? gt.data() : nullptr) != 0) return device_failed();
      } else if (!cloud_render_normals(gt_xyz, gt_normals.data(), n_gt, cam, o.splat, nullptr, gt.data(), err)) {
        return false;
      }
    }
    DpeNormalImage row;
    std::memset(&row, 0, sizeof row);
    row.id = ids[i];
    row.width = w;
    row.height = h;
    float* em = o.write_maps ? errmap.data() : nullptr;
    if (ctx) {
      if (dpe_normal_score(ctx, est.data(), from_maps ? gt.data() : nullptr, w, h, o.cos_tau, o.n_tau, &row.score, em) != 0)
        return device_failed();
    } else if (!normal_score(est.data(), gt.data(), w, h, o.cos_tau, o.n_tau, &row.score, em, err)) {
      return false;
    }
    if (o.write_maps) {
      const std::vector<int64_t> hw3 = {h, w, 3}, hw = {h, w};
      if (!write_npy((rf / "normal_gt.npy").string(), gt.data(), hw3, "<f4", 4, err) ||
          !write_npy((rf / "normal_error.npy").string(), errmap.data(), hw, "<f4", 4, err))
        return false;
    }
    done[i] = row;
    normal_add(&sum, row.score);
  }
  std::copy(done.begin(), done.end(), rows);
  *total = sum;
  return true;
}

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
  std::string err = "read_npy: bad argument";
  std::vector<float> v;
  int mw = 0, mh = 0;
  if (path && w && h && dpe_host::read_npy_f32x3(path, v, mw, mh, err)) {
    *w = mw;
    *h = mh;
    if (!data) return 0;
    if (cap >= v.size()) { std::memcpy(data, v.data(), v.size() * sizeof(float)); return 0; }
    err = "read_npy: room for fewer values than the file holds";
  }
  dpe_host::set_last_error(err);
  return 1;
}

int dpe_host_normal_eval(const DpeNormalEvalOptions* opt, const float* gt_xyz, size_t n_gt, DpeNormalImage* rows, size_t cap,
                         size_t* n_rows, DpeNormalScore* total) {
  return dpe_host::c_entry([&](std::string& err) { return opt && dpe_host::normal_eval(*opt, gt_xyz, n_gt, rows, cap, n_rows, total, err); },
                           "normal_eval: bad argument");
}

}  // extern "C"
