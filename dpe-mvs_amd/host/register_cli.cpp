// register_cli.cpp — bin/dpe_register: moves a source PLY onto a target PLY by point-to-point ICP
// (dpe_host_cloud_register, include/dpe_host.h states the loop) and writes the source transformed, colours kept.
//   dpe_register src.ply tgt.ply out.ply R [R ...] [--iters N] [--init t0 .. t11] [--gpu N | --cpu]
// R [R ...]: 1 to 4 radii, coarse to fine.  --init: the 12 numbers of a starting transform, row-major 3 x 4
// (default: the identity).  --gpu N (the default, N = 0) runs the steps on that device, --cpu on host threads: the
// same bytes.  Prints T (%.17g) and one line per stage; the reader and the writer are bin/dpe_voxel's.
// `python -m DPE_MVS.register` does the same.
#include <string>

#include "cli_common.h"

static int usage() {
  std::fprintf(stderr, "usage: dpe_register src.ply tgt.ply out.ply R [R ...] [--iters N] [--init t0 .. t11] [--gpu N | --cpu]\n");
  return 2;
}

int main(int argc, char** argv) {
  std::vector<const char*> pos;
  int gpu = 0;
  DpeCloudRegOptions opt{};
  opt.max_iters = 50;
  opt.tol = 1e-6;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (cli_device_option(argc, argv, i, gpu)) continue;
    if (a == "--iters" && i + 1 < argc) opt.max_iters = std::atoi(argv[++i]);
    else if (a == "--init" && i + 12 < argc) {
      for (int k = 0; k < 12; ++k) opt.init[k] = std::strtod(argv[++i], nullptr);
      opt.use_init = 1;
    }
    else if (a.rfind("--", 0) == 0) return usage();
    else pos.push_back(argv[i]);
  }
  if (pos.size() < 4 || pos.size() > 3 + DPE_CLOUD_MAX_RADII) return usage();
  for (size_t k = 3; k < pos.size(); ++k)
    if (!cli_number(pos[k], opt.radius[opt.n_radii++])) return usage();
  size_t n = 0, m = 0;
  int has_rgb = 0;
  std::vector<float> src, tgt;
  std::vector<uint8_t> rgb;
  DpeCloudReg reg;
  if (!cli_read_cloud(pos[0], src, n, &rgb, &has_rgb) || !cli_read_cloud(pos[1], tgt, m) ||
      dpe_host_cloud_register(src.data(), n, tgt.data(), m, &opt, gpu, &reg) != 0 ||
      dpe_host_cloud_transform(reg.T, src.data(), n, src.data()) != 0) {
    std::fprintf(stderr, "dpe_register: %s\n", dpe_pipeline_last_error());
    return 1;
  }
  std::vector<DpeFusedPoint> pts(n + 1);
  for (size_t r = 0; r < n; ++r) {
    const uint8_t* c = rgb.data() + 3 * r;
    pts[r] = DpeFusedPoint{src[3 * r], src[3 * r + 1], src[3 * r + 2], has_rgb ? (float)c[0] : 0.0f, has_rgb ? (float)c[1] : 0.0f,
                           has_rgb ? (float)c[2] : 0.0f};
  }
  if (dpe_host_write_point_cloud(pos[2], pts.data(), n) != 0) {
    std::fprintf(stderr, "dpe_register: cannot write %s\n", pos[2]);
    return 1;
  }
  for (int r = 0; r < 3; ++r)
    std::printf("T %.17g %.17g %.17g %.17g\n", reg.T[4 * r], reg.T[4 * r + 1], reg.T[4 * r + 2], reg.T[4 * r + 3]);
  for (int s = 0; s < reg.stages; ++s)
    std::printf("stage %d: radius %.9g, %d steps, %lld of %zu matched, rms %.9g, converged %d\n", s, (double)opt.radius[s], reg.iters[s],
                reg.matched[s], n, reg.rms[s], reg.converged[s]);
  return 0;
}
