// cloud_index.h — the hashed grid of one target cloud on the host (cloud_eval.cpp): built once, queried by
// dpe_host_cloud_nn, dpe_host_cloud_nn_index and every step of an ICP stage (cloud_register.cpp).  The grid and
// its arithmetic are csrc/cloud_dist.h's, which the kernels share.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../csrc/cloud_reg.h"

namespace dpe_host {

struct CloudIndex {
  dpe::CloudGrid g;
  float r2 = 0.0f;
  size_t finite = 0;              // finite target points; 0: no grid, every query gets (R2, -1)
  double origin[3] = {0, 0, 0};   // per-axis minimum of the finite target points (0 without any)
  std::vector<int> end;           // per bucket: the end of its points in st / sj
  std::vector<float> st;          // the target's points in bucket order
  std::vector<int32_t> sj;        // their original indices
  // false: "<who>: radius too small for the cloud's extent"
  bool build(const float* target, size_t m, float radius, const char* who, std::string& err);
  // out[i] = min(R2, min_j d2); idx (or nullptr): the j of the lexicographic minimum of (d2, j), -1 without one
  void query(const float* query, size_t n, float* out, int32_t* idx) const;
};

}  // namespace dpe_host
