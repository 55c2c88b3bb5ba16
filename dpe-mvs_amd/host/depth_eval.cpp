// depth_eval.cpp — the depth-map evaluation on the host: the render of a scan into one view and the score of
// one map as include/dpe_mvs.h states them (dpe_cloud_render_view, dpe_depth_score), with the pairwise tree
// taken literally, what is derived from a score, and the evaluation of a dense folder over either path.  The
// loops, map_eval.h's over DepthMetric, are the yardstick of the kernels (csrc/pass_render.h) and what runs without a
// GPU; the arithmetic is csrc/depth_eval.h's, which the kernels share.  No counterpart in the reference.
#include "map_eval.h"

#include <climits>
#include <cmath>

namespace fs = std::filesystem;

namespace dpe_host {

namespace {

using dpe::DepthMetric;

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

}  // namespace

bool cloud_render(const float* xyz, size_t n, const DpeCamera& cam, int splat, float* out, std::string& err) {
  if (!render_args_ok(xyz, n, &cam, splat, err)) return false;
  if (!out) { err = "cloud_render: bad argument"; return false; }
  const std::vector<uint32_t> zb = render_zbuffer<uint32_t>(xyz, n, cam, splat);
  for (size_t p = 0; p < zb.size(); ++p) {
    const uint32_t z = zb[p] == dpe::kDepthEmpty ? 0u : zb[p];
    std::memcpy(out + p, &z, sizeof z);
  }
  return true;
}

bool depth_score(const float* est, const float* gt, int w, int h, const float* tau, int n_tau, int mode, DpeDepthScore* out,
                 float* errmap, std::string& err) {
  if (!est || !gt || w < 1 || h < 1 || !out) { err = "depth_score: bad argument"; return false; }
  if (!score_args_ok(tau, n_tau, mode, err)) return false;
  dpe::DepthTaus T{};
  std::copy(tau, tau + n_tau, T.tau);
  T.n = n_tau;
  T.mode = mode;
  map_score<DepthMetric>(est, gt, w, h, T, out, errmap);
  return true;
}

void depth_stats(const DpeDepthScore& s, int n_tau, DpeDepthStats* out) {
  std::memset(out, 0, sizeof *out);
  stats_shares<DepthMetric>(s, n_tau, out->accuracy, out->completeness);
  if (s.n_both) {
    const double nb = (double)s.n_both;
    out->mae = s.sum_abs / nb;
    out->mre = s.sum_rel / nb;
    out->rmse = std::sqrt(s.sum_sq / nb);
  }
}

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

// map_eval's hooks
struct DepthEval {
  using Metric = DepthMetric;
  using Options = DpeDepthEvalOptions;
  using Image = DpeDepthImage;
  static constexpr const char *kWho = "depth_eval", *kMap = "depth.npy", *kGtName = "depth_gt.npy", *kErrName = "depth_error.npy";
  static bool read(const std::string& path, std::vector<float>& data, int& w, int& h, std::string& err) {
    return read_npy_f32(path, data, w, h, err);
  }
  bool args_ok(const Options& o, const float* xyz, size_t n, bool from_maps, std::string& err) {
    DpeCamera none{};
    none.width = none.height = 1;
    return score_args_ok(o.tau, o.n_tau, o.mode, err) && (from_maps || render_args_ok(xyz, n, &none, o.splat, err));
  }
  bool prepare(DpeContext* ctx, const Options&, const float* xyz, size_t n, std::string&) {
    return !ctx || dpe_cloud_render_stage(ctx, xyz, n) == 0;
  }
  int render_device(DpeContext* ctx, const DpeCamera& cam, const Options& o, float* gt) {
    return dpe_cloud_render_view(ctx, &cam, o.splat, gt);
  }
  bool render_host(const float* xyz, size_t n, const DpeCamera& cam, const Options& o, float* gt, std::string& err) {
    return cloud_render(xyz, n, cam, o.splat, gt, err);
  }
  int score_device(DpeContext* ctx, const float* est, const float* gt, int w, int h, const Options& o, DpeDepthScore* out, float* em) {
    return dpe_depth_score(ctx, est, gt, w, h, o.tau, o.n_tau, o.mode, out, em);
  }
  bool score_host(const float* est, const float* gt, int w, int h, const Options& o, DpeDepthScore* out, float* em, std::string& err) {
    return depth_score(est, gt, w, h, o.tau, o.n_tau, o.mode, out, em, err);
  }
};

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
  return dpe_host::read_npy_entry(dpe_host::read_npy_f32, path, data, cap, w, h);
}

int dpe_host_depth_eval_list(const char* dense_folder, const char* map_name, int* ids, size_t cap, size_t* n) {
  std::string err = "depth_eval: bad argument";
  std::vector<int> v;
  if (dense_folder && n && dpe_host::eval_list("depth_eval", dense_folder, dpe_host::map_name_or(map_name, dpe_host::DepthEval::kMap), v, err)) {
    *n = v.size();
    if (ids && cap >= v.size()) std::copy(v.begin(), v.end(), ids);
    return 0;
  }
  dpe_host::set_last_error(err);
  return 1;
}

int dpe_host_depth_eval(const DpeDepthEvalOptions* opt, const float* gt_xyz, size_t n_gt, DpeDepthImage* rows, size_t cap,
                        size_t* n_rows, DpeDepthScore* total) {
  dpe_host::DepthEval hooks;
  return dpe_host::c_entry([&](std::string& err) { return opt && dpe_host::map_eval(hooks, *opt, gt_xyz, n_gt, rows, cap, n_rows, total, err); },
                           "depth_eval: bad argument");
}

}  // extern "C"
