// cli_common.h — what the command lines bin/dpe_eval, bin/dpe_voxel, bin/dpe_register, bin/dpe_depth_eval and bin/dpe_normal_eval share:
// the device option, a PLY into vectors, a number that must be the whole argument, the JSON array writer, and the report
// of the two folder evaluations.
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

// The report of bin/dpe_depth_eval and bin/dpe_normal_eval after the tool's own first line: the table's header (the
// three columns `cols` of the metric in the widths of `col_fmt`, then `share`[k] and comp[k] per threshold), a row per
// image and the total through print_row(name, size, score, n_tau); with `json` the file as well: json_head writes the
// object's opening up to the thresholds, json_score one score's members.  Returns the tool's exit code
template <typename Image, typename Score, typename PrintRow, typename JsonHead, typename JsonScore>
int cli_eval_report(const char* tool, const char* col_fmt, const char* const (&cols)[3], const char* share, const Image* rows,
                    size_t n_img, const Score& total, int n_tau, const char* json, PrintRow print_row, JsonHead json_head,
                    JsonScore json_score) {
  std::printf("\n%8s %11s %10s %10s %10s", "image", "size", "n_gt", "n_est", "n_both");
  std::printf(col_fmt, cols[0], cols[1], cols[2]);
  for (int k = 0; k < n_tau; ++k) {
    char acc[32], comp[32];
    std::snprintf(acc, sizeof acc, "%s[%d]", share, k);
    std::snprintf(comp, sizeof comp, "comp[%d]", k);
    std::printf(" %10s %10s", acc, comp);
  }
  std::printf("\n");
  for (size_t i = 0; i < n_img; ++i) {
    char name[32], size[32];
    std::snprintf(name, sizeof name, "%08d", rows[i].id);
    std::snprintf(size, sizeof size, "%dx%d", rows[i].width, rows[i].height);
    print_row(name, size, rows[i].score, n_tau);
  }
  print_row("total", "-", total, n_tau);
  if (!json) return 0;
  FILE* f = std::fopen(json, "w");
  if (!f) { std::fprintf(stderr, "%s: cannot write %s\n", tool, json); return 1; }
  json_head(f);
  std::fprintf(f, ", \"images\": [");
  for (size_t i = 0; i < n_img; ++i) {
    std::fprintf(f, "%s{\"id\": %d, \"width\": %d, \"height\": %d, ", i ? ", " : "", rows[i].id, rows[i].width, rows[i].height);
    json_score(f, rows[i].score, n_tau);
    std::fprintf(f, "}");
  }
  std::fprintf(f, "], \"total\": {");
  json_score(f, total, n_tau);
  std::fprintf(f, "}}\n");
  std::fclose(f);
  return 0;
}
