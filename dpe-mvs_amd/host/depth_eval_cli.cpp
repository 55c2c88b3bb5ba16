// depth_eval_cli.cpp — bin/dpe_depth_eval: the depth maps of a dense folder against a ground-truth scan rendered
// into each view, or against ground-truth maps (dpe_host_depth_eval, include/dpe_host.h).
//   dpe_depth_eval dense_folder gt.ply tau [tau ...] [--relative] [--splat S] [--map depth.npy|depth_filtered.npy]
//                  [--maps] [--json FILE] [--gpu N | --cpu]
//   dpe_depth_eval dense_folder tau [tau ...] --gt-maps DIR [the same options but --splat]
// The images are the folders DPE/%08d that hold the map, in ascending id.  --relative compares |est - gt| with
// tau * gt instead of tau; --splat S renders every scan point over (2 S + 1)^2 pixels (0 to 8, default 0);
// --gt-maps DIR takes DIR/%08d.npy as the ground truth instead of a scan; --maps writes depth_gt.npy and
// depth_error.npy beside each map; --gpu N (the default, N = 0) renders and scores on that device, --cpu on the host:
// the same numbers.  Prints one table, a row per image and a total; --json also writes the counts and sums.
// `python -m DPE_MVS.depth_eval` prints the same table.
#include <string>

#include "cli_common.h"

static int usage() {
  std::fprintf(stderr, "usage: dpe_depth_eval dense_folder gt.ply tau [tau ...] [--relative] [--splat S] [--map NAME.npy]"
                       " [--gt-maps DIR] [--maps] [--json FILE] [--gpu N | --cpu]\n"
                       "       (with --gt-maps DIR no gt.ply is given)\n");
  return 2;
}

static void print_row(const char* name, const char* size, const DpeDepthScore& s, int n_tau) {
  DpeDepthStats d;
  dpe_host_depth_stats(&s, n_tau, &d);
  std::printf("%8s %11s %10lld %10lld %10lld %12.6g %12.6g %12.6g", name, size, s.n_gt, s.n_est, s.n_both, d.mae, d.mre, d.rmse);
  for (int k = 0; k < n_tau; ++k) std::printf(" %10.6f %10.6f", d.accuracy[k], d.completeness[k]);
  std::printf("\n");
}

static void json_score(FILE* f, const DpeDepthScore& s, int n_tau) {
  DpeDepthStats d;
  dpe_host_depth_stats(&s, n_tau, &d);
  std::fprintf(f, "\"n_px\": %lld, \"n_gt\": %lld, \"n_est\": %lld, \"n_both\": %lld, \"within\": [", s.n_px, s.n_gt, s.n_est, s.n_both);
  for (int k = 0; k < n_tau; ++k) std::fprintf(f, "%s%lld", k ? ", " : "", s.within[k]);
  std::fprintf(f, "], \"sum_abs\": %.17g, \"sum_rel\": %.17g, \"sum_sq\": %.17g, ", s.sum_abs, s.sum_rel, s.sum_sq);
  cli_json_array(f, "accuracy", d.accuracy, n_tau);
  std::fprintf(f, ", ");
  cli_json_array(f, "completeness", d.completeness, n_tau);
  std::fprintf(f, ", \"mae\": %.17g, \"mre\": %.17g, \"rmse\": %.17g", d.mae, d.mre, d.rmse);
}

int main(int argc, char** argv) {
  std::vector<const char*> pos;
  DpeDepthEvalOptions o{};
  o.gpu_index = 0;
  const char* json = nullptr;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (cli_device_option(argc, argv, i, o.gpu_index)) continue;
    if (a == "--relative") o.mode = DPE_DEPTH_TAU_REL;
    else if (a == "--maps") o.write_maps = 1;
    else if (a == "--splat" && i + 1 < argc) o.splat = std::atoi(argv[++i]);
    else if (a == "--map" && i + 1 < argc) o.map_name = argv[++i];
    else if (a == "--gt-maps" && i + 1 < argc) o.gt_maps_dir = argv[++i];
    else if (a == "--json" && i + 1 < argc) json = argv[++i];
    else if (a.rfind("--", 0) == 0) return usage();
    else pos.push_back(argv[i]);
  }
  const size_t first_tau = o.gt_maps_dir ? 1 : 2;
  if (pos.size() < first_tau + 1) return usage();
  o.dense_folder = pos[0];
  if (pos.size() - first_tau > DPE_DEPTH_MAX_TAU) {
    std::fprintf(stderr, "dpe_depth_eval: depth_score: 1 to 16 thresholds expected\n");
    return 1;
  }
  for (size_t k = first_tau; k < pos.size(); ++k)
    if (!cli_number(pos[k], o.tau[o.n_tau++])) return usage();
  std::vector<float> gt;
  size_t n = 0, n_img = 0;
  if (!o.gt_maps_dir && !cli_read_cloud(pos[1], gt, n)) {
    std::fprintf(stderr, "dpe_depth_eval: %s\n", dpe_pipeline_last_error());
    return 1;
  }
  if (dpe_host_depth_eval_list(o.dense_folder, o.map_name, nullptr, 0, &n_img) != 0) {
    std::fprintf(stderr, "dpe_depth_eval: %s\n", dpe_pipeline_last_error());
    return 1;
  }
  std::vector<DpeDepthImage> rows(n_img);
  DpeDepthScore total;
  if (dpe_host_depth_eval(&o, gt.data(), n, rows.data(), rows.size(), &n_img, &total) != 0) {
    std::fprintf(stderr, "dpe_depth_eval: %s\n", dpe_pipeline_last_error());
    return 1;
  }
  const char* map = o.map_name ? o.map_name : "depth.npy";
  std::printf("map %s, ground truth ", map);
  if (o.gt_maps_dir) std::printf("maps");
  else std::printf("cloud of %llu points, splat %d", (unsigned long long)n, o.splat);
  std::printf(", %s thresholds", o.mode == DPE_DEPTH_TAU_REL ? "relative" : "absolute");
  for (int k = 0; k < o.n_tau; ++k) std::printf(" %.9g", (double)o.tau[k]);
  return cli_eval_report("dpe_depth_eval", " %12s %12s %12s", {"mae", "mre", "rmse"}, "acc", rows.data(), n_img, total, o.n_tau, json,
                         print_row, [&](FILE* f) {
    std::fprintf(f, "{\"map\": \"%s\", \"relative\": %s, \"splat\": %d, \"n_gt_points\": %llu, \"tau\": [", map,
                 o.mode == DPE_DEPTH_TAU_REL ? "true" : "false", o.splat, (unsigned long long)n);
    for (int k = 0; k < o.n_tau; ++k) std::fprintf(f, "%s%.17g", k ? ", " : "", (double)o.tau[k]);
    std::fprintf(f, "]");
  }, json_score);
}
