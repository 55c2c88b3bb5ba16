// eval_cli.cpp — bin/dpe_eval: precision, recall and F-score of a reconstructed PLY against a ground-truth
// PLY (dpe_host_cloud_eval, include/dpe_host.h).
//   dpe_eval recon.ply gt.ply tau [tau...] [--radius R] [--gpu N | --cpu] [--json FILE]
// --gpu N (the default, N = 0) runs the distances on that device, --cpu on host threads: the same numbers.
// Prints one table; --json also writes the struct.  `python -m DPE_MVS.evaluate` prints the same table.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dpe_host.h"

static int usage() {
  std::fprintf(stderr, "usage: dpe_eval recon.ply gt.ply tau [tau...] [--radius R] [--gpu N | --cpu] [--json FILE]\n");
  return 2;
}

static bool read_cloud(const char* path, std::vector<float>& xyz, size_t& n) {
  if (dpe_host_read_point_cloud(path, nullptr, 0, &n) != 0) return false;
  xyz.resize(3 * n + 3);
  return dpe_host_read_point_cloud(path, xyz.data(), n, &n) == 0;
}

static void json_array(FILE* f, const char* name, const double* v, int n) {
  std::fprintf(f, "\"%s\": [", name);
  for (int k = 0; k < n; ++k) std::fprintf(f, "%s%.17g", k ? ", " : "", v[k]);
  std::fprintf(f, "]");
}

int main(int argc, char** argv) {
  std::vector<const char*> pos;
  float radius = 0.0f;
  int gpu = 0;
  const char* json = nullptr;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--cpu") gpu = -1;
    else if (a == "--gpu" && i + 1 < argc) gpu = std::atoi(argv[++i]);
    else if (a == "--radius" && i + 1 < argc) radius = std::strtof(argv[++i], nullptr);
    else if (a == "--json" && i + 1 < argc) json = argv[++i];
    else if (a.rfind("--", 0) == 0) return usage();
    else pos.push_back(argv[i]);
  }
  if (pos.size() < 3) return usage();
  std::vector<float> tau;
  for (size_t k = 2; k < pos.size(); ++k) {
    char* end = nullptr;
    tau.push_back(std::strtof(pos[k], &end));
    if (end == pos[k] || *end) return usage();
  }
  std::vector<float> recon, gt;
  size_t n = 0, m = 0;
  DpeCloudEval e;
  if (!read_cloud(pos[0], recon, n) || !read_cloud(pos[1], gt, m) ||
      dpe_host_cloud_eval(recon.data(), n, gt.data(), m, tau.data(), (int)tau.size(), radius, gpu, &e) != 0) {
    std::fprintf(stderr, "dpe_eval: %s\n", dpe_pipeline_last_error());
    return 1;
  }
  std::printf("recon %llu points (%llu dropped), gt %llu points (%llu dropped), radius %.9g\n", e.n_recon, e.dropped_recon,
              e.n_gt, e.dropped_gt, (double)e.radius);
  std::printf("%14s %10s %10s %10s\n", "tau", "precision", "recall", "fscore");
  for (int k = 0; k < e.n_tau; ++k)
    std::printf("%14.9g %10.6f %10.6f %10.6f\n", (double)e.tau[k], e.precision[k], e.recall[k], e.fscore[k]);
  std::printf("mean accuracy (truncated at the radius) %.9g\n", e.mean_accuracy_truncated);
  std::printf("mean completeness (truncated at the radius) %.9g\n", e.mean_completeness_truncated);
  if (json) {
    FILE* f = std::fopen(json, "w");
    if (!f) { std::fprintf(stderr, "dpe_eval: cannot write %s\n", json); return 1; }
    std::vector<double> t(e.tau, e.tau + e.n_tau);
    std::fprintf(f, "{\"n_tau\": %d, \"radius\": %.17g, ", e.n_tau, (double)e.radius);
    json_array(f, "tau", t.data(), e.n_tau); std::fprintf(f, ", ");
    json_array(f, "precision", e.precision, e.n_tau); std::fprintf(f, ", ");
    json_array(f, "recall", e.recall, e.n_tau); std::fprintf(f, ", ");
    json_array(f, "fscore", e.fscore, e.n_tau);
    std::fprintf(f, ", \"mean_accuracy_truncated\": %.17g, \"mean_completeness_truncated\": %.17g, ", e.mean_accuracy_truncated,
                 e.mean_completeness_truncated);
    std::fprintf(f, "\"n_recon\": %llu, \"n_gt\": %llu, \"dropped_recon\": %llu, \"dropped_gt\": %llu}\n", e.n_recon, e.n_gt,
                 e.dropped_recon, e.dropped_gt);
    std::fclose(f);
  }
  return 0;
}
