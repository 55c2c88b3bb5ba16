// pass_consistency.h — per-image consistency maps: how many source views agree with each pixel of a
// depth map, and the depth map filtered by that count.
//
// count[p] is the number of source views j for which the body of RunFusion's view loop
// (DPE.cpp:1312-1343) reaches `num_consistent++` WITHOUT the `masks[...]` tests and the `blocks` test:
// the reference depth is > 0, the projection lies inside view src[j] on a depth > 0, the reprojection
// error is < 2, the relative depth difference < 0.01 and GetAngle(n_ref, n_src) < 0.174533.  The masks
// are what makes RunFusion order-dependent; without them every pixel is independent, so the whole
// image runs here and 5 bytes per pixel go back to the host (the candidates of pass_fusion.h carry
// 16 * ns).  RunFusion's `dynamic_consistency` weight is not computed: it needs glibc's expf.
//
// Built from the fusions' functions: fz_world, fz_pixel (fusion_world.h) and tat_entry
// (pass_fusion_tat.h), so the arithmetic is theirs: the reference's expression order in single
// precision (-ffp-contract=off), the reprojection error in double rounded once.  The angle test
// needs no device acosf, as in pass_fusion_tat.h: the host passes D, the smallest float in [-1, 1]
// whose acosf is below 0.174533 (host/consistency.cpp), and the test is fz_angle_ok(dot, D).
#pragma once
#include "pass_fusion_tat.h"

namespace dpe {

constexpr int kConsistencyMaxSrc = 255;   // the count is one byte

// One thread per reference pixel; the loop over the views is wave-uniform (src, views and cams are
// read at uniform addresses).  count[p] as above; filtered[p] = count[p] >= min_views ? depth : 0.
__global__ void __launch_bounds__(256) k_consistency(const DpeCamera* __restrict__ cams,
                                                    const FusionViewDev* __restrict__ views, int ref,
                                                    const int* __restrict__ src, int ns, float dot_threshold,
                                                    int min_views, uint8_t* __restrict__ count,
                                                    float* __restrict__ filtered) {
  const FusionViewDev R = views[ref];
  const int L = R.w * R.h;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= L) return;
  const float ref_depth = R.depth[p];
  int n = 0;
  if (ref_depth > 0.0f) {
    const DpeCamera& rc = cams[ref];
    const int r = p / R.w, c = p - r * R.w;
    const FP3 X = fz_world(c, r, ref_depth, rc);
    for (int j = 0; j < ns; ++j) {
      const int s = src[j];
      const FusionViewDev S = views[s];
      const DpeCamera& sc = cams[s];
      int src_c, src_r;
      if (!fz_pixel(X, sc, S.w, S.h, src_c, src_r)) continue;
      const int sp = src_r * S.w + src_c;
      if (!(S.depth[sp] > 0.0f)) continue;
      const TatEntry e = tat_entry(R, rc, p, S, sc, sp);
      if (e.dist < 2.0f && e.depth < 0.01f && fz_angle_ok(e.dot, dot_threshold)) ++n;
    }
  }
  count[p] = (uint8_t)n;
  filtered[p] = n >= min_views ? ref_depth : 0.0f;
}

}  // namespace dpe
