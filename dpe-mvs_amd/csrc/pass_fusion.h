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
#include "fusion_world.h"        // fz_world, fz_pixel, fz_pair, fz_dot

namespace dpe {

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
  const float rn[3] = {R.normal[3 * (size_t)p], R.normal[3 * (size_t)p + 1], R.normal[3 * (size_t)p + 2]};
  for (int j = 0; j < ns; ++j) {
    int32_t o = -1;
    float e = 0.0f, rel = 0.0f, dot = 0.0f;
    const int s = src[j];
    const FusionViewDev S = views[s];
    const DpeCamera& sc = cams[s];
    int src_c, src_r;
    if (fz_pixel(X, sc, S.w, S.h, src_c, src_r)) {
      const int sp = src_r * S.w + src_c;
      const float sd = S.depth[sp];
      if (sd > 0.0f) {
        const FzPair d = fz_pair(c, r, ref_depth, rc, src_c, src_r, sd, sc);
        if (d.dist < 2.0f && d.depth < 0.01f) {   // the source normal is read for these only
          o = sp; e = d.dist; rel = d.depth;
          dot = fz_dot(rn, S.normal + 3 * (size_t)sp);
        }
      }
    }
    oi[j] = o;
    ov[3 * j] = e; ov[3 * j + 1] = rel; ov[3 * j + 2] = dot;
  }
}

}  // namespace dpe
