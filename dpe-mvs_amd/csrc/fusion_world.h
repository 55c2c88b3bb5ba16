// fusion_world.h — Get3DPointonWorld and ProjectCamera (DPE.cpp:1170-1206) on the device, in the
// reference's expression order and single precision (-ffp-contract=off).  Apart from the fusion
// kernels (pass_fusion.h) so that the per-image point cloud (pass_points.h) uses the same code.
#pragma once
#include "../../include/dpe_mvs.h"

namespace dpe {

struct FP3 { float x, y, z; };

// Get3DPointonWorld (DPE.cpp:1170-1194): camera centre from -R^T t
__device__ inline FP3 fz_world(int x, int y, float depth, const DpeCamera& cam) {
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
__device__ inline void fz_project(const FP3& X, const DpeCamera& cam, float& px, float& py, float& depth) {
  const float tx = cam.R[0] * X.x + cam.R[1] * X.y + cam.R[2] * X.z + cam.t[0];
  const float ty = cam.R[3] * X.x + cam.R[4] * X.y + cam.R[5] * X.z + cam.t[1];
  const float tz = cam.R[6] * X.x + cam.R[7] * X.y + cam.R[8] * X.z + cam.t[2];
  depth = cam.K[6] * tx + cam.K[7] * ty + cam.K[8] * tz;
  px = (cam.K[0] * tx + cam.K[1] * ty + cam.K[2] * tz) / depth;
  py = (cam.K[3] * tx + cam.K[4] * ty + cam.K[5] * tz) / depth;
}

}  // namespace dpe
