// normal_eval_cli.cpp — bin/dpe_normal_eval: the normal maps of a dense folder against the normals of a ground-truth
// scan rendered into each view, or against ground-truth normal maps (dpe_host_normal_eval, include/dpe_host.h).
//   dpe_normal_eval dense_folder gt.ply radius tau_deg [tau_deg ...] [--splat S] [--min-neighbours N] [--maps]
//                   [--json FILE] [--gpu N | --cpu]
//   dpe_normal_eval dense_folder tau_deg [tau_deg ...] --gt-normals DIR [--maps] [--json FILE] [--gpu N | --cpu]
// The images are the folders DPE/%08d that hold normal.npy, in ascending id.  The scan has no normals of its own: one
// is estimated per point by PCA over the points within `radius` (at least --min-neighbours of them, itself included,
// default 3; a point with fewer, or with collinear neighbours, has none), and the normal of the point that wins a pixel's z-buffer is
// that pixel's ground truth, turned towards the camera.  --splat S renders every scan point over (2 S + 1)^2 pixels
// (0 to 8, default 0); --gt-normals DIR takes DIR/%08d.npy, f32 [h][w][3] in the world frame, as the ground truth;
// --maps writes normal_gt.npy and normal_error.npy beside each map; --gpu N (the default, N = 0) runs on that
// device, --cpu on the host: the same numbers.  The thresholds are angles in degrees.  Prints one table, a row per image
// and a total; --json also writes the counts and sums.  `python -m DPE_MVS.normal_eval` prints the same table.
#include <string>

#include "cli_common.h"

static int usage() {
  std::fprintf(stderr, "usage: dpe_normal_eval dense_folder gt.ply radius tau_deg [tau_deg ...] [--splat S] [--min-neighbours N]"
                       " [--gt-normals DIR] [--maps] [--json FILE] [--gpu N | --cpu]\n"
                       "       (with --gt-normals DIR neither gt.ply nor radius is given)\n");
  return 2;
}

static void print_row(const char* name, const char* size, const DpeNormalScore& s, int n_tau) {
  DpeNormalStats d;
  dpe_host_normal_stats(&s, n_tau, &d);
  std::printf("%8s %11s %10lld %10lld %10lld %12.6g %10.1f %10.4f", name, size, s.n_gt, s.n_est, s.n_both, d.mean_cos_dist,
              d.median_deg, d.mean_deg);
  for (int k = 0; k < n_tau; ++k) std::printf(" %10.6f %10.6f", d.share[k], d.completeness[k]);
  std::printf("\n");
}

static void json_score(FILE* f, const DpeNormalScore& s, int n_tau) {
  DpeNormalStats d;
  dpe_host_normal_stats(&s, n_tau, &d);
  std::fprintf(f, "\"n_px\": %lld, \"n_gt\": %lld, \"n_est\": %lld, \"n_both\": %lld, \"within\": [", s.n_px, s.n_gt, s.n_est, s.n_both);
  for (int k = 0; k < n_tau; ++k) std::fprintf(f, "%s%lld", k ? ", " : "", s.within[k]);
  std::fprintf(f, "], \"hist\": [");
  for (int b = 0; b < DPE_NORMAL_BINS; ++b) std::fprintf(f, "%s%lld", b ? ", " : "", s.hist[b]);
  std::fprintf(f, "], \"sum_dist\": %.17g, \"sum_dist_sq\": %.17g, ", s.sum_dist, s.sum_dist_sq);
  cli_json_array(f, "share", d.share, n_tau);
  std::fprintf(f, ", ");
  cli_json_array(f, "completeness", d.completeness, n_tau);
  std::fprintf(f, ", \"mean_cos_dist\": %.17g, \"median_deg\": %.17g, \"mean_deg\": %.17g", d.mean_cos_dist, d.median_deg, d.mean_deg);
}

int main(int argc, char** argv) {
  std::vector<const char*> pos;
  DpeNormalEvalOptions o{};
  o.gpu_index = 0;
  o.min_nb = 3;
  const char* json = nullptr;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (cli_device_option(argc, argv, i, o.gpu_index)) continue;
    if (a == "--maps") o.write_maps = 1;
    else if (a == "--splat" && i + 1 < argc) o.splat = std::atoi(argv[++i]);
    else if (a == "--min-neighbours" && i + 1 < argc) o.min_nb = std::atoi(argv[++i]);
    else if (a == "--gt-normals" && i + 1 < argc) o.gt_maps_dir = argv[++i];
    else if (a == "--json" && i + 1 < argc) json = argv[++i];
    else if (a.rfind("--", 0) == 0) return usage();
    else pos.push_back(argv[i]);
  }
  const size_t first_tau = o.gt_maps_dir ? 1 : 3;
  if (pos.size() < first_tau + 1) return usage();
  o.dense_folder = pos[0];
  if (!o.gt_maps_dir && !cli_number(pos[2], o.radius)) return usage();
  if (pos.size() - first_tau > DPE_NORMAL_MAX_TAU) {
    std::fprintf(stderr, "dpe_normal_eval: normal_score: 1 to 16 thresholds expected\n");
    return 1;
  }
  float deg[DPE_NORMAL_MAX_TAU];
  for (size_t k = first_tau; k < pos.size(); ++k) {
    if (!cli_number(pos[k], deg[o.n_tau])) return usage();
    o.cos_tau[o.n_tau] = dpe_host_normal_cos((double)deg[o.n_tau]);
    ++o.n_tau;
  }
  std::vector<float> gt;
  size_t n = 0, n_img = 0;
  if (!o.gt_maps_dir && !cli_read_cloud(pos[1], gt, n)) {
    std::fprintf(stderr, "dpe_normal_eval: %s\n", dpe_pipeline_last_error());
    return 1;
  }
  // sized for every image that holds the map; dpe_host_normal_eval lists them again and reports what it refuses
  if (dpe_host_depth_eval_list(o.dense_folder, "normal.npy", nullptr, 0, &n_img) != 0) n_img = 0;
  std::vector<DpeNormalImage> rows(n_img);
  DpeNormalScore total;
  if (dpe_host_normal_eval(&o, gt.data(), n, rows.data(), rows.size(), &n_img, &total) != 0) {
    std::fprintf(stderr, "dpe_normal_eval: %s\n", dpe_pipeline_last_error());
    return 1;
  }
  std::printf("map normal.npy, ground truth ");
  if (o.gt_maps_dir) std::printf("maps");
  else std::printf("cloud of %llu points, radius %.9g, min neighbours %d, splat %d", (unsigned long long)n, (double)o.radius, o.min_nb, o.splat);
  std::printf(", thresholds in degrees");
  for (int k = 0; k < o.n_tau; ++k) std::printf(" %.9g", (double)deg[k]);
  return cli_eval_report("dpe_normal_eval", " %12s %10s %10s", {"cos_dist", "median", "mean"}, "within", rows.data(), n_img, total,
                         o.n_tau, json, print_row, [&](FILE* f) {
    std::fprintf(f, "{\"map\": \"normal.npy\", \"splat\": %d, \"radius\": %.9g, \"min_neighbours\": %d, \"n_gt_points\": %llu, \"tau_deg\": [",
                 o.splat, (double)o.radius, o.min_nb, (unsigned long long)n);
    for (int k = 0; k < o.n_tau; ++k) std::fprintf(f, "%s%.9g", k ? ", " : "", (double)deg[k]);
    std::fprintf(f, "]");
  }, json_score);
}
