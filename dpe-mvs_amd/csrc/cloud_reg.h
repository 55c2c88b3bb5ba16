// cloud_reg.h — the arithmetic of the rigid registration (dpe_cloud_icp_step of include/dpe_mvs.h, which states
// the contract) that the host (host/cloud_register.cpp) shares with the kernels (pass_register.h): the image of
// a point under a transform, the 16 terms of a matched pair, and the running pair (d2, index) of the match.
// Plain C++, -ffp-contract=off like everything here: every operation below is one rounded operation.
#pragma once
#include "cloud_dist.h"

namespace dpe {

constexpr int kIcpTerms = 16;   // d2, a[3], b[3], a[r] * b[c]

// one row of x' = [R | t] x: (float)(((T[0]*x + T[1]*y) + T[2]*z) + T[3]) in double, in this order
DPE_CHD float icp_apply_row(const double* T, float x, float y, float z) {
  double s = T[0] * (double)x;
  const double u = T[1] * (double)y;
  s = s + u;
  const double w = T[2] * (double)z;
  s = s + w;
  s = s + T[3];
  return (float)s;
}

// the image of a finite point under T (row-major 3 x 4)
DPE_CHD void icp_apply(const double* T, float x, float y, float z, float* o) {
  o[0] = icp_apply_row(T, x, y, z);
  o[1] = icp_apply_row(T + 4, x, y, z);
  o[2] = icp_apply_row(T + 8, x, y, z);
}

// the running pair of the match: (s, j) replaces (best, best_j) when it is lexicographically smaller.  From
// (R2, -1) only s < R2 can set an index, and a NaN s never does.
DPE_CHD void icp_take(float s, int j, float& best, int& best_j) {
  if (s < best || (s == best && j < best_j)) { best = s; best_j = j; }
}

// the 16 terms of source point p matched to target point g at squared distance d2; os / ot: the per-axis minima
// of the finite points of either cloud, so a, b >= +0.0 and no term is ever -0.0
DPE_CHD void icp_terms(const float* p, const float* g, float d2, const double* os, const double* ot, double* t) {
  t[0] = (double)d2;
  for (int r = 0; r < 3; ++r) {
    t[1 + r] = (double)p[r] - os[r];
    t[4 + r] = (double)g[r] - ot[r];
  }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) t[7 + 3 * r + c] = t[1 + r] * t[4 + c];
}

}  // namespace dpe
