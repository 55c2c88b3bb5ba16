// cli_common.h — what the command lines bin/dpe_eval, bin/dpe_voxel, bin/dpe_register, bin/dpe_depth_eval and bin/dpe_normal_eval share:
// the device option, a PLY into vectors, a number that must be the whole argument, and the JSON array writer.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/dpe_host.h"

// --gpu N | --cpu at argv[i]: sets gpu (N, or -1 for the host path), steps i over N and returns true
inline bool cli_device_option(int argc, char** argv, int& i, int& gpu) {
  if (std::strcmp(argv[i], "--cpu") == 0) { gpu = -1; return true; }
  if (std::strcmp(argv[i], "--gpu") == 0 && i + 1 < argc) { gpu = std::atoi(argv[++i]); return true; }
  return false;
}

// the float that is all of `s`; false for anything else
inline bool cli_number(const char* s, float& v) {
  char* end = nullptr;
  v = std::strtof(s, &end);
  return end != s && !*end;
}

// the positions of a PLY (and its colours when rgb is not null; *has_rgb says whether it holds any); on failure the
// message is dpe_pipeline_last_error's
inline bool cli_read_cloud(const char* path, std::vector<float>& xyz, size_t& n, std::vector<uint8_t>* rgb = nullptr,
                           int* has_rgb = nullptr) {
  int has = 0;
  if (dpe_host_read_point_cloud_rgb(path, nullptr, nullptr, 0, &n, &has) != 0) return false;
  xyz.resize(3 * n + 3);
  if (rgb) rgb->resize(3 * n + 3);
  if (dpe_host_read_point_cloud_rgb(path, xyz.data(), rgb ? rgb->data() : nullptr, n, &n, &has) != 0) return false;
  if (has_rgb) *has_rgb = has;
  return true;
}

// "name": [v0, v1, ...] with every digit of the doubles
inline void cli_json_array(FILE* f, const char* name, const double* v, int n) {
  std::fprintf(f, "\"%s\": [", name);
  for (int k = 0; k < n; ++k) std::fprintf(f, "%s%.17g", k ? ", " : "", v[k]);
  std::fprintf(f, "]");
}
