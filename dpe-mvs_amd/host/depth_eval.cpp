// depth_eval.cpp — the depth-map evaluation on the host: the render of a scan into one view and the score of
// one map as include/dpe_mvs.h states them (dpe_cloud_render_view, dpe_depth_score), with the pairwise tree
// taken literally, what is derived from a score, and the evaluation of a dense folder over either path.  The
// loops are the yardstick of the kernels (csrc/pass_render.h) and what runs without a GPU; the arithmetic is
// csrc/depth_eval.h's, which the kernels share.  No counterpart in the reference.
#include "host.h"
#include "pairwise_tree.h"
#include "parallel.h"
#include "../csrc/depth_eval.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <filesystem>
#include <string>
#include <vector>

namespace fs = std::filesystem;

namespace dpe_host {

namespace {

using dpe::kDepthTerms;

// points [i0, i1) into the z-buffer zb (bit patterns)
void render_range(const float* xyz, size_t i0, size_t i1, const DpeCamera& cam, int s, uint32_t* zb) {
  const int w = cam.width, h = cam.height;
  for (size_t i = i0; i < i1; ++i) {
    int cx, cy;
    uint32_t z;
    if (!dpe::depth_point(cam, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], cx, cy, z)) continue;
    const int x0 = std::max(0, cx - s), x1 = std::min(w - 1, cx + s);
    const int y0 = std::max(0, cy - s), y1 = std::min(h - 1, cy + s);
    for (int y = y0; y <= y1; ++y) {
      uint32_t* row = zb + (size_t)y * (size_t)w;
      for (int x = x0; x <= x1; ++x)
        if (z < row[x]) row[x] = z;
    }
  }
}

bool render_args_ok(const float* xyz, size_t n, const DpeCamera* cam, int splat, std::string& err) {
  if (n > (size_t)INT_MAX || (!xyz && n) || !cam) { err = "cloud_render: bad argument"; return false; }
  if (cam->width < 1 || cam->height < 1) { err = "cloud_render: the camera's width and height must be at least 1"; return false; }
  if (splat < 0 || splat > DPE_DEPTH_MAX_SPLAT) { err = "cloud_render: the splat half-width must be 0 to 8"; return false; }
  return true;
}

bool score_args_ok(const float* tau, int n_tau, int mode, std::string& err) {
  if (!tau || n_tau < 1 || n_tau > DPE_DEPTH_MAX_TAU) { err = "depth_score: 1 to 16 thresholds expected"; return false; }
  for (int k = 0; k < n_tau; ++k)
    if (!std::isfinite(tau[k]) || !(tau[k] >= 0.0f)) { err = "depth_score: a threshold is negative or not finite"; return false; }
  if (mode != DPE_DEPTH_TAU_ABS && mode != DPE_DEPTH_TAU_REL) { err = "depth_score: unknown threshold mode"; return false; }
  return true;
}

constexpr size_t kRenderPerThread = 1u << 16;   // fewer points than this per thread are not worth a z-buffer

}  // namespace

bool cloud_render(const float* xyz, size_t n, const DpeCamera& cam, int splat, float* out, std::string& err) {
  if (!render_args_ok(xyz, n, &cam, splat, err)) return false;
  if (!out) { err = "cloud_render: bad argument"; return false; }
  const size_t npx = (size_t)cam.width * (size_t)cam.height;
  const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)host_threads(), n / kRenderPerThread));
  // one z-buffer of bit patterns per thread over its share of the points, merged by minimum below
  std::vector<uint32_t> zb((size_t)nt * npx, dpe::kDepthEmpty);
  run_on_threads(nt, [&](int t) { render_range(xyz, n * t / nt, n * (t + 1) / nt, cam, splat, zb.data() + (size_t)t * npx); });
  for (size_t p = 0; p < npx; ++p) {
    uint32_t z = zb[p];
    for (int t = 1; t < nt; ++t) z = std::min(z, zb[(size_t)t * npx + p]);
    if (z == dpe::kDepthEmpty) z = 0u;
    std::memcpy(out + p, &z, sizeof z);
  }
  return true;
}

bool depth_score(const float* est, const float* gt, int w, int h, const float* tau, int n_tau, int mode, DpeDepthScore* out,
                 float* errmap, std::string& err) {
  if (!est || !gt || w < 1 || h < 1 || !out) { err = "depth_score: bad argument"; return false; }
  if (!score_args_ok(tau, n_tau, mode, err)) return false;
  DpeDepthScore s;
  std::memset(&s, 0, sizeof s);   // the structs are compared as bytes
  const size_t npx = (size_t)w * (size_t)h;
  PairwiseTree<kDepthTerms> tree;
  for (size_t i = 0; i < npx; ++i) {
    const dpe::DepthPixel p = dpe::depth_pixel(est[i], gt[i]);
    s.n_gt += p.gt_ok;
    s.n_est += p.est_ok;
    s.n_both += p.both;
    for (int k = 0; k < n_tau; ++k) s.within[k] += dpe::depth_hit(p, gt[i], tau[k], mode);
    double t[kDepthTerms];
    dpe::depth_terms(p, t);
    tree.push(t);
    if (errmap) errmap[i] = dpe::depth_error_code(p);
  }
  double sums[kDepthTerms];
  tree.finish(sums);
  s.n_px = (long long)npx;
  s.sum_abs = sums[0];
  s.sum_rel = sums[1];
  s.sum_sq = sums[2];
  *out = s;
  return true;
}

void depth_stats(const DpeDepthScore& s, int n_tau, DpeDepthStats* out) {
  std::memset(out, 0, sizeof *out);
  const double nb = (double)s.n_both, ng = (double)s.n_gt;
  for (int k = 0; k < n_tau && k < DPE_DEPTH_MAX_TAU; ++k) {
    out->accuracy[k] = s.n_both ? (double)s.within[k] / nb : 0.0;
    out->completeness[k] = s.n_gt ? (double)s.within[k] / ng : 0.0;
  }
  if (s.n_both) {
    out->mae = s.sum_abs / nb;
    out->mre = s.sum_rel / nb;
    out->rmse = std::sqrt(s.sum_sq / nb);
  }
}

void depth_add(DpeDepthScore* total, const DpeDepthScore& s) {
  total->n_px += s.n_px;
  total->n_gt += s.n_gt;
  total->n_est += s.n_est;
  total->n_both += s.n_both;
  for (int k = 0; k < DPE_DEPTH_MAX_TAU; ++k) total->within[k] += s.within[k];
  total->sum_abs = total->sum_abs + s.sum_abs;
  total->sum_rel = total->sum_rel + s.sum_rel;
  total->sum_sq = total->sum_sq + s.sum_sq;
}

namespace {

const char* map_name_of(const char* name) { return name && *name ? name : "depth.npy"; }

}  // namespace

// the image ids of the folder: DPE/<8 digits> that hold the map, ascending
bool eval_list(const char* who, const std::string& dense, const std::string& map, std::vector<int>& ids, std::string& err) {
  const fs::path root = fs::path(dense) / "DPE";
  std::error_code ec;
  if (!fs::is_directory(root, ec)) { err = std::string(who) + ": no DPE folder in " + dense; return false; }
  for (fs::directory_iterator it(root, ec), end; !ec && it != end; it.increment(ec)) {
    const std::string name = it->path().filename().string();
    if (name.size() != 8 || !std::all_of(name.begin(), name.end(), [](char c) { return c >= '0' && c <= '9'; })) continue;
    if (!fs::is_regular_file(it->path() / map, ec)) continue;
    ids.push_back(std::atoi(name.c_str()));
  }
  std::sort(ids.begin(), ids.end());
  if (ids.empty()) { err = std::string(who) + ": no such map: no DPE/<id>/" + map + " in " + dense; return false; }
  return true;
}

// the camera of image `id` at the size w x h of its map: ReadCamera, the intrinsics scaled from the image's size
// (map_view's arithmetic, pipeline.cpp)
bool map_camera(const std::string& dense, int id, int w, int h, DpeCamera& cam, std::string& err) {
  if (!read_camera((fs::path(dense) / "cams" / (fmt_index(id) + "_cam.txt")).string(), cam, err)) return false;
  GrayImage img;
  if (!read_gray((fs::path(dense) / "images" / (fmt_index(id) + ".jpg")).string(), img, err)) return false;
  if (img.w != w || img.h != h) scale_intrinsics(cam, w / (float)img.w, h / (float)img.h);
  cam.width = w;
  cam.height = h;
  return true;
}

namespace {

bool depth_eval(const DpeDepthEvalOptions& o, const float* gt_xyz, size_t n_gt, DpeDepthImage* rows, size_t cap, size_t* n_rows,
                DpeDepthScore* total, std::string& err) {
  if (!o.dense_folder || !n_rows || !total || (!rows && cap)) { err = "depth_eval: bad argument"; return false; }
  if (!score_args_ok(o.tau, o.n_tau, o.mode, err)) return false;
  const bool from_maps = o.gt_maps_dir && *o.gt_maps_dir;
  DpeCamera none{};
  none.width = none.height = 1;
  if (!from_maps && !render_args_ok(gt_xyz, n_gt, &none, o.splat, err)) return false;
  const std::string dense = o.dense_folder, map = map_name_of(o.map_name);
  std::vector<int> ids;
  if (!eval_list("depth_eval", dense, map, ids, err)) return false;
  *n_rows = ids.size();
  if (cap < ids.size()) { err = "depth_eval: room for fewer rows than images"; return false; }
  OwnedContext own(o.gpu_index, "depth_eval", err);
  if (!own.ok) return false;
  DpeContext* ctx = own.ctx;
  auto device_failed = [&]() { err = std::string("depth_eval: ") + dpe_last_error(); return false; };
  if (ctx && !from_maps && dpe_cloud_render_stage(ctx, gt_xyz, n_gt) != 0) return device_failed();
  DpeDepthScore sum;
  std::memset(&sum, 0, sizeof sum);
  std::vector<float> est, gt, errmap;
  std::vector<DpeDepthImage> done(ids.size());   // a failure leaves the caller's rows alone
  for (size_t i = 0; i < ids.size(); ++i) {
    const fs::path rf = fs::path(dense) / "DPE" / fmt_index(ids[i]);
    int w = 0, h = 0;
    if (!read_npy_f32((rf / map).string(), est, w, h, err)) return false;
    const size_t npx = (size_t)w * (size_t)h;
    const bool want_gt = !ctx || from_maps || o.write_maps;   // the ground truth on the host
    if (want_gt) gt.resize(npx);
    if (o.write_maps) errmap.resize(npx);
    if (from_maps) {
      int gw = 0, gh = 0;
      const std::string path = (fs::path(o.gt_maps_dir) / (fmt_index(ids[i]) + ".npy")).string();
      if (!read_npy_f32(path, gt, gw, gh, err)) return false;
      if (gw != w || gh != h) { err = "depth_eval: size mismatch: " + path + " is not of the size of " + (rf / map).string(); return false; }
    } else {
      DpeCamera cam;
      if (!map_camera(dense, ids[i], w, h, cam, err)) return false;
      if (ctx) {
        if (dpe_cloud_render_view(ctx, &cam, o.splat, want_gt ? gt.data() : nullptr) != 0) return device_failed();
      } else if (!cloud_render(gt_xyz, n_gt, cam, o.splat, gt.data(), err)) {
        return false;
      }
    }
    DpeDepthImage row;
    std::memset(&row, 0, sizeof row);
    row.id = ids[i];
    row.width = w;
    row.height = h;
    float* em = o.write_maps ? errmap.data() : nullptr;
    if (ctx) {
      if (dpe_depth_score(ctx, est.data(), from_maps ? gt.data() : nullptr, w, h, o.tau, o.n_tau, o.mode, &row.score, em) != 0)
        return device_failed();
    } else if (!depth_score(est.data(), gt.data(), w, h, o.tau, o.n_tau, o.mode, &row.score, em, err)) {
      return false;
    }
    if (o.write_maps) {
      const std::vector<int64_t> hw = {h, w};
      if (!write_npy((rf / "depth_gt.npy").string(), gt.data(), hw, "<f4", 4, err) ||
          !write_npy((rf / "depth_error.npy").string(), errmap.data(), hw, "<f4", 4, err))
        return false;
    }
    done[i] = row;
    depth_add(&sum, row.score);
  }
  std::copy(done.begin(), done.end(), rows);
  *total = sum;
  return true;
}

}  // namespace

}  // namespace dpe_host

extern "C" {

int dpe_host_cloud_render(const float* xyz, size_t n, const DpeCamera* cam, int splat, float* depth_out) {
  return dpe_host::c_entry([&](std::string& err) { return cam && dpe_host::cloud_render(xyz, n, *cam, splat, depth_out, err); },
                           "cloud_render: bad argument");
}

int dpe_host_depth_score(const float* est, const float* gt, int w, int h, const float* tau, int n_tau, int mode,
                         DpeDepthScore* out, float* err_or_null) {
  return dpe_host::c_entry(
      [&](std::string& err) { return dpe_host::depth_score(est, gt, w, h, tau, n_tau, mode, out, err_or_null, err); });
}

void dpe_host_depth_stats(const DpeDepthScore* s, int n_tau, DpeDepthStats* out) {
  if (s && out) dpe_host::depth_stats(*s, n_tau, out);
}

int dpe_host_read_npy_f32(const char* path, float* data, size_t cap, int* w, int* h) {
  std::string err = "read_npy: bad argument";
  std::vector<float> v;
  int mw = 0, mh = 0;
  if (path && w && h && dpe_host::read_npy_f32(path, v, mw, mh, err)) {
    *w = mw;
    *h = mh;
    if (!data) return 0;
    if (cap >= v.size()) { std::memcpy(data, v.data(), v.size() * sizeof(float)); return 0; }
    err = "read_npy: room for fewer values than the file holds";
  }
  dpe_host::set_last_error(err);
  return 1;
}

int dpe_host_depth_eval_list(const char* dense_folder, const char* map_name, int* ids, size_t cap, size_t* n) {
  std::string err = "depth_eval: bad argument";
  std::vector<int> v;
  if (dense_folder && n && dpe_host::eval_list("depth_eval", dense_folder, dpe_host::map_name_of(map_name), v, err)) {
    *n = v.size();
    if (ids && cap >= v.size()) std::copy(v.begin(), v.end(), ids);
    return 0;
  }
  dpe_host::set_last_error(err);
  return 1;
}

int dpe_host_depth_eval(const DpeDepthEvalOptions* opt, const float* gt_xyz, size_t n_gt, DpeDepthImage* rows, size_t cap,
                        size_t* n_rows, DpeDepthScore* total) {
  return dpe_host::c_entry([&](std::string& err) { return opt && dpe_host::depth_eval(*opt, gt_xyz, n_gt, rows, cap, n_rows, total, err); },
                           "depth_eval: bad argument");
}

}  // extern "C"
