// fusion_world.h — the arithmetic of the fusion section that the host (host/fusion*.cpp, host/consistency.cpp,
// host/points.cpp) shares with the kernels (pass_fusion.h, pass_fusion_tat.h, pass_consistency.h, pass_points.h)
// and with the map evaluations (depth_eval.h): Get3DPointonWorld and ProjectCamera (DPE.cpp:1170-1206), the source
// pixel of a projection, and what a pair (reference pixel, source pixel) is tested on.  Plain C++ in the
// reference's expression order, -ffp-contract=off on both sides: every operation is one rounded single-precision
// operation with IEEE division, unless a double is written.  acos stays on the host (get_angle, host/fusion_tat.cpp).
#pragma once
#include "../../include/dpe_mvs.h"
#include "chd.h"   // DPE_CHD

namespace dpe {

struct FP3 { float x, y, z; };

// Get3DPointonWorld (DPE.cpp:1170-1194): camera centre from -R^T t
DPE_CHD FP3 fz_world(int x, int y, float depth, const DpeCamera& cam) {
  FP3 p, t, C;
  p.x = depth * ((float)x - cam.K[2]) / cam.K[0];
  p.y = depth * ((float)y - cam.K[5]) / cam.K[4];
  p.z = depth;
  t.x = cam.R[0] * p.x + cam.R[3] * p.y + cam.R[6] * p.z;
  t.y = cam.R[1] * p.x + cam.R[4] * p.y + cam.R[7] * p.z;
  t.z = cam.R[2] * p.x + cam.R[5] * p.y + cam.R[8] * p.z;
  C.x = -(cam.R[0] * cam.t[0] + cam.R[3] * cam.t[1] + cam.R[6] * cam.t[2]);
  C.y = -(cam.R[1] * cam.t[0] + cam.R[4] * cam.t[1] + cam.R[7] * cam.t[2]);
  C.z = -(cam.R[2] * cam.t[0] + cam.R[5] * cam.t[1] + cam.R[8] * cam.t[2]);
  return FP3{t.x + C.x, t.y + C.y, t.z + C.z};
}

// ProjectCamera (DPE.cpp:1196-1206)
DPE_CHD void fz_project(const FP3& X, const DpeCamera& cam, float& px, float& py, float& depth) {
  const float tx = cam.R[0] * X.x + cam.R[1] * X.y + cam.R[2] * X.z + cam.t[0];
  const float ty = cam.R[3] * X.x + cam.R[4] * X.y + cam.R[5] * X.z + cam.t[1];
  const float tz = cam.R[6] * X.x + cam.R[7] * X.y + cam.R[8] * X.z + cam.t[2];
  depth = cam.K[6] * tx + cam.K[7] * ty + cam.K[8] * tz;
  px = (cam.K[0] * tx + cam.K[1] * ty + cam.K[2] * tz) / depth;
  py = (cam.K[3] * tx + cam.K[4] * ty + cam.K[5] * tz) / depth;
}

// The pixel (c, r) = (int(px + 0.5f), int(py + 0.5f)) of a projection (DPE.cpp:1318-1321), taken only for
// px + 0.5, py + 0.5 in (-1, size) of a w x h image: the in-range test on the float, so NaN / huge projections
// are rejected the same way as on the reference's host (where they convert to INT_MIN).  False when the
// projection lies outside.  The one copy of this rule.
DPE_CHD bool fz_pixel(float px, float py, int w, int h, int& c, int& r) {
  const float fx = px + 0.5f, fy = py + 0.5f;
  if (!(fx > -1.0f && fx < (float)w && fy > -1.0f && fy < (float)h)) return false;
  c = (int)fx; r = (int)fy;
  return true;
}

// the pixel of the projection of X into a w x h view with camera `cam`
DPE_CHD bool fz_pixel(const FP3& X, const DpeCamera& cam, int w, int h, int& c, int& r) {
  float px, py, pd;
  fz_project(X, cam, px, py, pd);
  return fz_pixel(px, py, w, h, c, r);
}

// What reference pixel (c, r) at ref_depth and the source pixel (src_c, src_r) at src_depth are apart
// (DPE.cpp:1326-1333): the source pixel goes to the world and back into the reference view.
struct FzPair { float dist, depth; };   // reprojection error, relative depth difference
DPE_CHD FzPair fz_pair(int c, int r, float ref_depth, const DpeCamera& rc, int src_c, int src_r, float src_depth,
                       const DpeCamera& sc) {
  const FP3 Y = fz_world(src_c, src_r, src_depth, sc);
  float tx, ty, pd2;
  fz_project(Y, rc, tx, ty, pd2);
  const float dx = (float)c - tx, dy = (float)r - ty;
  FzPair e;
  // DPE.cpp:1331 sqrt(pow(c - x, 2) + pow(r - y, 2)): pow(float, int) promotes to double, so the squares, the
  // sum and the root are double, rounded to float once
  e.dist = (float)__builtin_sqrt((double)dx * dx + (double)dy * dy);
  e.depth = __builtin_fabsf(pd2 - ref_depth) / ref_depth;
  return e;
}

// the dot product of the two normals, what GetAngle (DPE.cpp:1208-1217) takes the acos of
DPE_CHD float fz_dot(const float* rn, const float* sn) { return rn[0] * sn[0] + rn[1] * sn[1] + rn[2] * sn[2]; }

// `GetAngle(n_ref, n_src) < T` without acos: D is the smallest float in [-1, 1] whose acosf is below T
// (angle_dot_threshold, host/fusion_tat.cpp), and GetAngle returns 0 for a NaN acosf
DPE_CHD bool fz_angle_ok(float dot, float D) { return !(dot >= -1.0f && dot <= 1.0f) || dot >= D; }

}  // namespace dpe
