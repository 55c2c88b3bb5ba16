// voxel_cli.cpp — bin/dpe_voxel: thins a PLY to one point per voxel (dpe_cloud_voxel / dpe_host_cloud_voxel,
// include/dpe_mvs.h states the contract) and keeps its colours.
//   dpe_voxel in.ply out.ply V [--gpu N | --cpu]
// --gpu N (the default, N = 0) runs on that device, --cpu the serial host loop: the same bytes.  The output is
// written by dpe_host_write_point_cloud (a file without colours gets black); the point counts before and after
// go to stderr.  `python -m DPE_MVS.voxel` does the same.
#include <string>

#include "cli_common.h"

static int usage() {
  std::fprintf(stderr, "usage: dpe_voxel in.ply out.ply V [--gpu N | --cpu]\n");
  return 2;
}

int main(int argc, char** argv) {
  std::vector<const char*> pos;
  int gpu = 0;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (cli_device_option(argc, argv, i, gpu)) continue;
    if (a.rfind("--", 0) == 0) return usage();
    else pos.push_back(argv[i]);
  }
  if (pos.size() != 3) return usage();
  float v = 0.0f;
  if (!cli_number(pos[2], v)) return usage();
  size_t n = 0, k = 0;
  int has_rgb = 0;
  std::vector<float> xyz;
  std::vector<uint8_t> rgb;
  if (!cli_read_cloud(pos[0], xyz, n, &rgb, &has_rgb)) {
    std::fprintf(stderr, "dpe_voxel: %s\n", dpe_pipeline_last_error());
    return 1;
  }
  std::vector<float> out(3 * n + 3);
  std::vector<uint8_t> out_rgb(3 * n + 3);
  std::vector<int32_t> first(n + 1), count(n + 1);
  const uint8_t* colours = has_rgb ? rgb.data() : nullptr;
  if (gpu < 0) {
    if (dpe_host_cloud_voxel(xyz.data(), n, colours, v, out.data(), out_rgb.data(), first.data(), count.data(), n, &k) != 0) {
      std::fprintf(stderr, "dpe_voxel: %s\n", dpe_pipeline_last_error());
      return 1;
    }
  } else {
    DpeContext* ctx = dpe_create(gpu);
    const int rc = ctx ? dpe_cloud_voxel(ctx, xyz.data(), n, colours, v, out.data(), out_rgb.data(), first.data(), count.data(), n, &k)
                       : DPE_ERR_HIP;
    if (rc != 0) std::fprintf(stderr, "dpe_voxel: %s\n", dpe_last_error());
    if (ctx) dpe_destroy(ctx);
    if (rc != 0) return 1;
  }
  std::vector<DpeFusedPoint> pts(k + 1);
  for (size_t r = 0; r < k; ++r) {
    const uint8_t* c = out_rgb.data() + 3 * r;
    pts[r] = DpeFusedPoint{out[3 * r], out[3 * r + 1], out[3 * r + 2], has_rgb ? (float)c[0] : 0.0f, has_rgb ? (float)c[1] : 0.0f,
                           has_rgb ? (float)c[2] : 0.0f};
  }
  if (dpe_host_write_point_cloud(pos[1], pts.data(), k) != 0) {
    std::fprintf(stderr, "dpe_voxel: cannot write %s\n", pos[1]);
    return 1;
  }
  std::fprintf(stderr, "dpe_voxel: %zu points -> %zu points (voxel %.9g)\n", n, k, (double)v);
  return 0;
}
