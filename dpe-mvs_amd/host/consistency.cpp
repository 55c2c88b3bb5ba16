// consistency.cpp — the consistency maps on the host: per reference pixel, the number of source views
// that pass RunFusion's three tests (DPE.cpp:1312-1343 with the `masks[...]` tests and the `blocks` test
// removed), and the depth map filtered by that count.  The serial double loop as the reference would
// write it, calling acosf itself: the yardstick of the device kernel (csrc/pass_consistency.h) and what
// DpePipelineOptions.consistency runs with a fusion_runner hook (no GPU).  Single precision in the
// reference's expression order; the in-range test of the projection on the float, as every fusion here.
// RunFusion's dynamic_consistency weight (exp) is not part of it.
#include "host.h"

#include <string>

namespace dpe_host {
namespace {
const float kAngleMax = 0.174533f;   // DPE.cpp:1335
}

void consistency_image(const DpeFusionView* views, int ref, const int* src, int ns, int min_views, uint8_t* count,
                       float* filtered) {
  const DpeFusionView& R = views[ref];
  const int cols = R.width, rows = R.height;
  for (int r = 0; r < rows; ++r) {
    for (int c = 0; c < cols; ++c) {
      const size_t p = (size_t)r * cols + c;
      const float ref_depth = R.depth[p];
      int num_consistent = 0;
      if (ref_depth > 0.0f) {
        const float* ref_normal = R.normal + 3 * p;
        const FP3 PointX = fz_world(c, r, ref_depth, R.cam);
        for (int j = 0; j < ns; ++j) {
          const DpeFusionView& S = views[src[j]];
          int src_c, src_r;
          if (!fz_pixel(PointX, S.cam, S.width, S.height, src_c, src_r)) continue;
          const size_t sp = (size_t)src_r * S.width + src_c;
          const float src_depth = S.depth[sp];
          if (!(src_depth > 0.0f)) continue;
          const FzPair d = fz_pair(c, r, ref_depth, R.cam, src_c, src_r, src_depth, S.cam);
          const float reproj_error = d.dist, relative_depth_diff = d.depth;
          const float angle = get_angle(fz_dot(ref_normal, S.normal + 3 * sp));
          if (reproj_error < 2.0f && relative_depth_diff < 0.01f && angle < kAngleMax) num_consistent++;
        }
      }
      if (count) count[p] = (uint8_t)num_consistent;
      if (filtered) filtered[p] = num_consistent >= min_views ? ref_depth : 0.0f;
    }
  }
}

bool consistency_dot_threshold(float& D, std::string& err) {
  switch (angle_dot_threshold(kAngleMax, D)) {
    case DotThreshold::kOk: return true;
    case DotThreshold::kNonePasses: err = "consistency: no dot product passes the angle test"; return false;
    default: err = "consistency: the angle threshold does not verify"; return false;
  }
}

bool consistency_args_ok(int n_views, int ref, const int* src, int ns, int min_views, std::string& err) {
  if (n_views < 1 || ns < 0 || (ns > 0 && !src)) { err = "consistency: bad argument"; return false; }
  if (ns > 255) { err = "consistency: more than 255 source views"; return false; }
  if (min_views < 1 || min_views > 255) { err = "consistency: min_views outside 1..255"; return false; }
  if (ref < 0 || ref >= n_views) { err = "consistency: bad reference view"; return false; }
  for (int j = 0; j < ns; ++j) {
    if (src[j] < 0 || src[j] >= n_views) { err = "consistency: bad source view"; return false; }
    if (src[j] == ref) { err = "consistency: the reference view is among its sources"; return false; }
  }
  return true;
}

}  // namespace dpe_host

extern "C" {

int dpe_host_consistency(const DpeFusionView* views, int n_views, int ref, const int* src, int ns, int min_views,
                         uint8_t* count, float* depth_filtered) {
  std::string err;
  if (!views || !dpe_host::consistency_args_ok(n_views, ref, src, ns, min_views, err)) return 1;
  for (int i = 0; i < n_views; ++i)
    if (views[i].width < 1 || views[i].height < 1 || !views[i].depth || !views[i].normal) return 1;
  dpe_host::consistency_image(views, ref, src, ns, min_views, count, depth_filtered);
  return 0;
}

int dpe_host_consistency_dot_threshold(float* D) {
  std::string err;
  if (!D) return 1;
  return dpe_host::consistency_dot_threshold(*D, err) ? 0 : 1;
}

int dpe_host_consistency_angle_test(float dot) { return dpe_host::get_angle(dot) < dpe_host::kAngleMax ? 1 : 0; }

}  // extern "C"
