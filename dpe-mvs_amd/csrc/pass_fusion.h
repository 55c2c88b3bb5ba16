// pass_fusion.h — RunFusion's per-pixel projection tests (DPE.cpp:1303-1343) on the GPU.
//
// RunFusion walks the reference pixels of every image in order, projects each into its source
// views, and keeps a point when enough views agree; a kept point masks the source pixels it used,
// so the walk is order-dependent.  Everything except the masks is independent per (pixel, view):
// the two projections, the reprojection error, the relative depth difference and the normal dot
// product.  This kernel computes exactly that part, one thread per reference pixel, in the
// reference's expression order and precision (-ffp-contract=off, IEEE division and sqrt; single
// precision except the reprojection error, whose pow() promotes to double), and
// the host finishes with the masks, the angle test (acosf), the weights (expf) and the colours in
// the reference's serial order (host/fusion.cpp).
#pragma once
#include "../../include/dpe_mvs.h"
#include "dpe_fusion_types.h"   // FusionViewDev
#include "fusion_world.h"        // fz_world, fz_project

namespace dpe {

// The source pixel (src_c, src_r) = (int(x + 0.5f), int(y + 0.5f)) of the projection of X into view S
// (DPE.cpp:1318-1321), taken only for x + 0.5, y + 0.5 in (-1, size): the in-range test on the float,
// so NaN / huge projections are rejected the same way as on the reference's host (where they convert
// to INT_MIN).  False when the projection lies outside.  The one copy of this test: the candidates
// below, the Tanks-and-Temples hit (pass_fusion_tat.h) and the consistency count (pass_consistency.h).
__device__ inline bool fz_pixel(const FP3& X, const FusionViewDev& S, const DpeCamera& sc, int& src_c, int& src_r) {
  float px, py, pd;
  fz_project(X, sc, px, py, pd);
  const float fx = px + 0.5f, fy = py + 0.5f;
  if (!(fx > -1.0f && fx < (float)S.w && fy > -1.0f && fy < (float)S.h)) return false;
  src_c = (int)fx; src_r = (int)fy;
  return true;
}

// idx[p*ns + j]: source pixel (row-major) when the projection of reference pixel p lands inside
// source view src[j] on a positive depth with reprojection error < 2 and relative depth difference
// < 0.01, else -1.  val[(p*ns + j)*3 + {0, 1, 2}] = (reprojection error, relative depth difference,
// normal dot product) of those candidates.
__global__ void __launch_bounds__(256) k_fusion_candidates(const DpeCamera* __restrict__ cams,
                                                          const FusionViewDev* __restrict__ views, int ref,
                                                          const int* __restrict__ src, int ns,
                                                          int32_t* __restrict__ idx, float* __restrict__ val) {
  const FusionViewDev R = views[ref];
  const int L = R.w * R.h;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= L) return;
  const int r = p / R.w, c = p - r * R.w;
  int32_t* oi = idx + (size_t)p * ns;
  float* ov = val + (size_t)p * ns * 3;
  const float ref_depth = R.depth[p];
  if (!(ref_depth > 0.0f)) {
    for (int j = 0; j < ns; ++j) oi[j] = -1;
    return;
  }
  const DpeCamera& rc = cams[ref];
  const FP3 X = fz_world(c, r, ref_depth, rc);
  const float n0 = R.normal[3 * (size_t)p], n1 = R.normal[3 * (size_t)p + 1], n2 = R.normal[3 * (size_t)p + 2];
  for (int j = 0; j < ns; ++j) {
    int32_t o = -1;
    float e = 0.0f, rel = 0.0f, dot = 0.0f;
    const int s = src[j];
    const FusionViewDev S = views[s];
    const DpeCamera& sc = cams[s];
    int src_c, src_r;
    if (fz_pixel(X, S, sc, src_c, src_r)) {
      const int sp = src_r * S.w + src_c;
      const float sd = S.depth[sp];
      if (sd > 0.0f) {
        const FP3 Y = fz_world(src_c, src_r, sd, sc);
        float tx, ty, pd2;
        fz_project(Y, rc, tx, ty, pd2);
        const float dx = (float)c - tx, dy = (float)r - ty;
        // DPE.cpp:1331 sqrt(pow(c - x, 2) + pow(r - y, 2)): pow(float, int) promotes to double, so the
        // squares, the sum and the root are double, rounded to float once
        const float re = (float)__builtin_sqrt((double)dx * dx + (double)dy * dy);
        const float rl = __builtin_fabsf(pd2 - ref_depth) / ref_depth;
        if (re < 2.0f && rl < 0.01f) {
          o = sp; e = re; rel = rl;
          const float* sn = S.normal + 3 * (size_t)sp;
          dot = n0 * sn[0] + n1 * sn[1] + n2 * sn[2];
        }
      }
    }
    oi[j] = o;
    ov[3 * j] = e; ov[3 * j + 1] = rel; ov[3 * j + 2] = dot;
  }
}

}  // namespace dpe
