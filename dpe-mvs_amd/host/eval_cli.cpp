// eval_cli.cpp — bin/dpe_eval: precision, recall and F-score of a reconstructed PLY against a ground-truth
// PLY (dpe_host_cloud_eval, include/dpe_host.h).
//   dpe_eval recon.ply gt.ply tau [tau...] [--radius R] [--voxel V] [--crop x0 y0 z0 x1 y1 z1] [--gpu N | --cpu] [--json FILE]
//            [--register R [R ...]] [--register-iters N] [--register-init t0 .. t11]
// --voxel V down-samples both clouds to one point per voxel of edge V before they are scored, --crop keeps the
// points inside the box first (dpe_host_cloud_eval_prep); with either the table gets a first line naming them.
// --register R [R ...] (1 to 4 radii, coarse to fine: the numbers that follow it) first moves the reconstruction onto
// the ground truth by point-to-point ICP (dpe_host_cloud_eval_reg; --register-iters: steps per radius, default 50;
// --register-init: a starting transform, row-major 3 x 4); the table then begins with the radii, the final rms and T.
// --gpu N (the default, N = 0) runs the distances on that device, --cpu on host threads: the same numbers.
// Prints one table; --json also writes the struct.  `python -m DPE_MVS.evaluate` prints the same table.
#include <string>

#include "cli_common.h"

static int usage() {
  std::fprintf(stderr, "usage: dpe_eval recon.ply gt.ply tau [tau...] [--radius R] [--voxel V] [--crop x0 y0 z0 x1 y1 z1]"
                       " [--gpu N | --cpu] [--json FILE] [--register R [R ...]] [--register-iters N] [--register-init t0 .. t11]\n");
  return 2;
}

int main(int argc, char** argv) {
  std::vector<const char*> pos;
  float radius = 0.0f;
  int gpu = 0;
  const char* json = nullptr;
  DpeCloudPrep prep{};
  bool prepared = false, have_voxel = false, registered = false;
  DpeCloudRegOptions ropt{};
  ropt.max_iters = 50;
  ropt.tol = 1e-6;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (cli_device_option(argc, argv, i, gpu)) continue;
    if (a == "--radius" && i + 1 < argc) radius = std::strtof(argv[++i], nullptr);
    else if (a == "--json" && i + 1 < argc) json = argv[++i];
    else if (a == "--voxel" && i + 1 < argc) { prep.voxel = std::strtof(argv[++i], nullptr); prepared = have_voxel = true; }
    else if (a == "--crop" && i + 6 < argc) {
      for (int k = 0; k < 3; ++k) prep.crop_lo[k] = std::strtof(argv[++i], nullptr);
      for (int k = 0; k < 3; ++k) prep.crop_hi[k] = std::strtof(argv[++i], nullptr);
      prep.use_crop = 1;
      prepared = true;
    }
    else if (a == "--register") {
      registered = true;
      while (i + 1 < argc && ropt.n_radii < DPE_CLOUD_MAX_RADII) {   // the numbers that follow
        float r = 0.0f;
        if (!cli_number(argv[i + 1], r)) break;
        ropt.radius[ropt.n_radii++] = r;
        ++i;
      }
    }
    else if (a == "--register-iters" && i + 1 < argc) ropt.max_iters = std::atoi(argv[++i]);
    else if (a == "--register-init" && i + 12 < argc) {
      for (int k = 0; k < 12; ++k) ropt.init[k] = std::strtod(argv[++i], nullptr);
      ropt.use_init = 1;
    }
    else if (a.rfind("--", 0) == 0) return usage();
    else pos.push_back(argv[i]);
  }
  if (pos.size() < 3) return usage();
  if (have_voxel && !(prep.voxel > 0.0f)) {   // 0 means "none" in the block; asked for on the command line it is an error
    std::fprintf(stderr, "dpe_eval: cloud_eval: the voxel edge is not a finite positive number\n");
    return 1;
  }
  std::vector<float> tau(pos.size() - 2);
  for (size_t k = 2; k < pos.size(); ++k)
    if (!cli_number(pos[k], tau[k - 2])) return usage();
  std::vector<float> recon, gt;
  size_t n = 0, m = 0;
  DpeCloudEval e;
  DpeCloudReg reg{};
  if (!cli_read_cloud(pos[0], recon, n) || !cli_read_cloud(pos[1], gt, m) ||
      (registered ? dpe_host_cloud_eval_reg(recon.data(), n, gt.data(), m, tau.data(), (int)tau.size(), radius, gpu,
                                            prepared ? &prep : nullptr, &ropt, &reg, &e)
                  : dpe_host_cloud_eval_prep(recon.data(), n, gt.data(), m, tau.data(), (int)tau.size(), radius, gpu,
                                             prepared ? &prep : nullptr, &e)) != 0) {
    std::fprintf(stderr, "dpe_eval: %s\n", dpe_pipeline_last_error());
    return 1;
  }
  if (registered) {
    std::printf("registered: radii");
    for (int s = 0; s < reg.stages; ++s) std::printf(" %.9g", (double)ropt.radius[s]);
    std::printf(", rms %.9g\n", reg.rms[reg.stages - 1]);
    for (int r = 0; r < 3; ++r)
      std::printf("T %.17g %.17g %.17g %.17g\n", reg.T[4 * r], reg.T[4 * r + 1], reg.T[4 * r + 2], reg.T[4 * r + 3]);
  }
  if (prepared) {
    std::printf("prepared: voxel %.9g, crop", (double)prep.voxel);
    if (prep.use_crop)
      std::printf(" [%.9g %.9g %.9g] to [%.9g %.9g %.9g]", (double)prep.crop_lo[0], (double)prep.crop_lo[1], (double)prep.crop_lo[2],
                  (double)prep.crop_hi[0], (double)prep.crop_hi[1], (double)prep.crop_hi[2]);
    else
      std::printf(" none");
    std::printf(", from recon %llu points, gt %llu points\n", prep.n_recon_in, prep.n_gt_in);
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
    cli_json_array(f, "tau", t.data(), e.n_tau); std::fprintf(f, ", ");
    cli_json_array(f, "precision", e.precision, e.n_tau); std::fprintf(f, ", ");
    cli_json_array(f, "recall", e.recall, e.n_tau); std::fprintf(f, ", ");
    cli_json_array(f, "fscore", e.fscore, e.n_tau);
    std::fprintf(f, ", \"mean_accuracy_truncated\": %.17g, \"mean_completeness_truncated\": %.17g, ", e.mean_accuracy_truncated,
                 e.mean_completeness_truncated);
    std::fprintf(f, "\"n_recon\": %llu, \"n_gt\": %llu, \"dropped_recon\": %llu, \"dropped_gt\": %llu", e.n_recon, e.n_gt,
                 e.dropped_recon, e.dropped_gt);
    if (prepared) {
      if (have_voxel) std::fprintf(f, ", \"voxel\": %.17g", (double)prep.voxel);
      else std::fprintf(f, ", \"voxel\": null");
      std::fprintf(f, ", \"n_recon_in\": %llu, \"n_gt_in\": %llu, \"crop\": ", prep.n_recon_in, prep.n_gt_in);
      if (prep.use_crop)
        std::fprintf(f, "[[%.17g, %.17g, %.17g], [%.17g, %.17g, %.17g]]", (double)prep.crop_lo[0], (double)prep.crop_lo[1],
                     (double)prep.crop_lo[2], (double)prep.crop_hi[0], (double)prep.crop_hi[1], (double)prep.crop_hi[2]);
      else
        std::fprintf(f, "null");
    }
    if (registered) {
      std::fprintf(f, ", \"registration\": {\"T\": [");
      for (int r = 0; r < 3; ++r)
        std::fprintf(f, "%s[%.17g, %.17g, %.17g, %.17g]", r ? ", " : "", reg.T[4 * r], reg.T[4 * r + 1], reg.T[4 * r + 2], reg.T[4 * r + 3]);
      std::fprintf(f, "], \"stages\": [");
      for (int s = 0; s < reg.stages; ++s)
        std::fprintf(f, "%s{\"radius\": %.17g, \"iters\": %d, \"matched\": %lld, \"rms\": %.17g, \"converged\": %d}", s ? ", " : "",
                     (double)ropt.radius[s], reg.iters[s], reg.matched[s], reg.rms[s], reg.converged[s]);
      std::fprintf(f, "]}");
    }
    std::fprintf(f, "}\n");
    std::fclose(f);
  }
  return 0;
}
