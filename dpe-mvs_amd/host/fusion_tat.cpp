// fusion_tat.cpp — the two Tanks-and-Temples fusions, RunFusion_TAT_Intermediate (DPE.cpp:1372-1540)
// and RunFusion_TAT_advanced (DPE.cpp:1542-1689), selected by DpePipelineOptions.fusion_mode.
//
// Two paths over the same views:
//  * the serial loops as the reference writes them (tat_intermediate_serial / tat_advanced_serial):
//    problems in pair.txt order, pixels row-major, the per-view `diff` entries declared OUTSIDE the
//    pixel loops and never reset (DPE.cpp:1462, :1626), so a view that does not hit at a pixel keeps
//    the entry of the last pixel where it did.  Single precision in the reference's expression order.
//    This is the yardstick of the tests, and what runs when the caller supplies a fusion_runner hook
//    (no GPU), when a problem lists its own image among its sources, or when two problems share an
//    image id (masks[ref] would then be read while it is written);
//  * the device path over dpe_fusion_tat_begin / dpe_fusion_tat_image (csrc/pass_fusion_tat.h): one
//    image at a time on the GPU, only the points come back, and the copy-out of image i runs beside
//    the kernels of image i + 1.
// The angle test of the Intermediate variant, `GetAngle(n_ref, n_src) < k * angle_grad + angle_base`,
// goes to the device as a table of dot-product thresholds (tat_thresholds), built with the same
// get_angle the serial loop calls.
#include "host.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

namespace dpe_host {

// GetAngle (DPE.cpp:1208-1217) from the dot product
float get_angle(float dot_product) {
  float angle = std::acos(dot_product);
  if (angle != angle) return 0.0f;
  return angle;
}

namespace {

const float kAngleBase = 0.06981317007977318f;   // 4 degree (DPE.cpp:1380)
const float kAngleGrad = 0.05235987755982988f;   // 3 degree (DPE.cpp:1381)

float angle_threshold(int k) { return k * kAngleGrad + kAngleBase; }   // DPE.cpp:1508

using Plan = FusionPlan;   // host.h

// What both loops do per (pixel, source view) before the entry is written (DPE.cpp:1481-1496): the
// source pixel when the rounded projection lies inside the view (the in-range test on the float, as
// the GPU kernels take it: NaN and huge projections are rejected), is not masked and has a depth.
struct Hit { bool ok; int src_r, src_c; float reproj_error, relative_depth_diff, angle; };
Hit project_and_test(const FP3& PointX, int r, int c, float ref_depth, const float* ref_normal, const FusionView& R,
                     const FusionView& S) {
  Hit h{false, 0, 0, 0.0f, 0.0f, 0.0f};
  int src_c, src_r;
  if (!fz_pixel(PointX, S.view.cam, S.view.width, S.view.height, src_c, src_r)) return h;
  const size_t sp = (size_t)src_r * S.view.width + src_c;
  if (S.mask[sp] == 1) return h;
  const float src_depth = S.view.depth[sp];
  if (src_depth <= 0.0) return h;
  const FzPair d = fz_pair(c, r, ref_depth, R.view.cam, src_c, src_r, src_depth, S.view.cam);
  h.reproj_error = d.dist;
  h.relative_depth_diff = d.depth;
  h.angle = get_angle(fz_dot(ref_normal, S.view.normal + 3 * sp));
  h.ok = true; h.src_r = src_r; h.src_c = src_c;
  return h;
}

void tat_intermediate_serial(std::vector<FusionView>& views, const Plan& pl, std::vector<FusedPoint>& PointCloud) {
  const float dist_base = 0.25f;
  const float depth_base = 1.0f / 3500.0f;
  const float angle_base = kAngleBase;
  const float angle_grad = kAngleGrad;
  struct CostData {
    float dist = FLT_MAX, depth = FLT_MAX, angle = FLT_MAX;
    int src_r = 0, src_c = 0;
    bool use = false;
  };
  const int num_images = (int)views.size();
  for (int i = 0; i < num_images; ++i) {
    FusionView& R = views[pl.refs[i]];
    const bool use_block = !R.block.empty();
    const int cols = R.view.width, rows = R.view.height;
    const int num_ngb = (int)pl.srcs[i].size();
    std::vector<CostData> diff(num_ngb, CostData());   // outside the pixel loops: entries go stale, as in the reference
    for (int r = 0; r < rows; ++r) {
      for (int c = 0; c < cols; ++c) {
        const size_t p = (size_t)r * cols + c;
        if (use_block && R.block[p] < 128) continue;
        const float ref_depth = R.view.depth[p];
        if (ref_depth <= 0.0) continue;
        const float* ref_normal = R.view.normal + 3 * p;
        const FP3 PointX = fz_world(c, r, ref_depth, R.view.cam);
        for (int j = 0; j < num_ngb; ++j) {
          const Hit h = project_and_test(PointX, r, c, ref_depth, ref_normal, R, views[pl.srcs[i][j]]);
          if (!h.ok) continue;
          diff[j].dist = h.reproj_error;
          diff[j].depth = h.relative_depth_diff;
          diff[j].angle = h.angle;
          diff[j].src_r = h.src_r;
          diff[j].src_c = h.src_c;
        }
        for (int k = 2; k <= num_ngb; ++k) {
          int count = 0;
          for (int j = 0; j < num_ngb; ++j) {
            diff[j].use = false;
            if (diff[j].dist < k * dist_base && diff[j].depth < k * depth_base && diff[j].angle < (k * angle_grad + angle_base)) {
              count++;
              diff[j].use = true;
            }
          }
          if (count >= k) {
            float consistent_Color[3] = {(float)R.bgr[3 * p], (float)R.bgr[3 * p + 1], (float)R.bgr[3 * p + 2]};
            for (int j = 0; j < num_ngb; ++j) {
              if (diff[j].use) {
                const FusionView& S = views[pl.srcs[i][j]];
                const size_t sp = (size_t)diff[j].src_r * S.view.width + diff[j].src_c;
                consistent_Color[0] += (float)S.bgr[3 * sp];
                consistent_Color[1] += (float)S.bgr[3 * sp + 1];
                consistent_Color[2] += (float)S.bgr[3 * sp + 2];
              }
            }
            consistent_Color[0] /= (count + 1.0f);
            consistent_Color[1] /= (count + 1.0f);
            consistent_Color[2] /= (count + 1.0f);
            PointCloud.push_back(FusedPoint{PointX.x, PointX.y, PointX.z, consistent_Color[0], consistent_Color[1],
                                            consistent_Color[2]});
            R.mask[p] = 1;
            break;
          }
        }
      }
    }
  }
}

void tat_advanced_serial(std::vector<FusionView>& views, const Plan& pl, std::vector<FusedPoint>& PointCloud) {
  const float dist_base = 0.25f;
  const float depth_base = 1.0f / 3000.0f;
  struct CostData {
    float dist = FLT_MAX, depth = FLT_MAX, angle = FLT_MAX;
  };
  const int num_images = (int)views.size();
  for (int i = 0; i < num_images; ++i) {
    FusionView& R = views[pl.refs[i]];
    const bool use_block = !R.block.empty();
    const int cols = R.view.width, rows = R.view.height;
    const int num_ngb = (int)pl.srcs[i].size();
    std::vector<CostData> diff(num_ngb, CostData());   // outside the pixel loops, as in the reference
    for (int r = 0; r < rows; ++r) {
      for (int c = 0; c < cols; ++c) {
        const size_t p = (size_t)r * cols + c;
        if (use_block && R.block[p] < 128) continue;
        const float ref_depth = R.view.depth[p];
        if (ref_depth <= 0.0) continue;
        const float* ref_normal = R.view.normal + 3 * p;
        const FP3 PointX = fz_world(c, r, ref_depth, R.view.cam);
        const float consistent_Color[3] = {(float)R.bgr[3 * p], (float)R.bgr[3 * p + 1], (float)R.bgr[3 * p + 2]};
        for (int j = 0; j < num_ngb; ++j) {
          const Hit h = project_and_test(PointX, r, c, ref_depth, ref_normal, R, views[pl.srcs[i][j]]);
          if (!h.ok) continue;
          diff[j].dist = h.reproj_error;
          diff[j].depth = h.relative_depth_diff;
          diff[j].angle = h.angle;
        }
        for (int k = 2; k <= num_ngb; ++k) {
          int count = 0;
          for (int j = 0; j < num_ngb; ++j) {
            if (diff[j].dist < k * dist_base && diff[j].depth < k * depth_base) count++;
          }
          if (count >= k) {
            PointCloud.push_back(FusedPoint{PointX.x, PointX.y, PointX.z, consistent_Color[0], consistent_Color[1],
                                            consistent_Color[2]});
            R.mask[p] = 1;
            break;
          }
        }
      }
    }
  }
}

// the default path: every image on the device, in order
bool tat_device(std::vector<FusionView>& views, const Plan& pl, int mode, DpeContext* ctx, std::vector<FusedPoint>& cloud,
                std::string& err) {
  const int n = (int)views.size();
  auto fail = [&](const char* what) { err = std::string(what) + ": " + dpe_last_error(); return false; };
  std::vector<DpeFusionView> dv(n);
  std::vector<const uint8_t*> bgr(n), block(n);
  size_t cap = 1;
  for (int i = 0; i < n; ++i) {
    dv[i] = views[i].view;
    bgr[i] = views[i].bgr.data();
    block[i] = views[i].block.empty() ? nullptr : views[i].block.data();
    cap = std::max(cap, (size_t)views[i].view.width * views[i].view.height);
  }
  float D[32] = {0};
  if (mode == DPE_FUSION_TAT_INTERMEDIATE && !tat_thresholds(D, 32, err)) return false;
  if (dpe_fusion_stage(ctx, dv.data(), n) != DPE_OK) return fail("dpe_fusion_stage");
  if (dpe_fusion_tat_begin(ctx, bgr.data(), block.data()) != DPE_OK) return fail("dpe_fusion_tat_begin");
  // the points of image i land in buf[i & 1] while image i + 1 runs; page-locked when the runtime allows
  std::vector<FusedPoint> buf[2] = {std::vector<FusedPoint>(cap), std::vector<FusedPoint>(cap)};
  PinnedRange pins[2];
  for (int k = 0; k < 2; ++k) pins[k].pin(buf[k].data(), cap * sizeof(FusedPoint));
  size_t before = 0;   // points of the image before, whose copy the next call completes
  bool ok = true;
  for (int i = 0; i < n && ok; ++i) {
    size_t cnt = 0;
    ok = dpe_fusion_tat_image(ctx, mode, pl.refs[i], pl.srcs[i].data(), (int)pl.srcs[i].size(), D, buf[i & 1].data(), cap,
                              &cnt) == DPE_OK;
    if (!ok) { fail("dpe_fusion_tat_image"); cnt = 0; }
    cloud.insert(cloud.end(), buf[(i + 1) & 1].begin(), buf[(i + 1) & 1].begin() + before);
    before = cnt;
  }
  if (dpe_fusion_tat_wait(ctx) != DPE_OK && ok) ok = fail("dpe_fusion_tat_wait");   // before the buffers go
  if (ok) cloud.insert(cloud.end(), buf[(n + 1) & 1].begin(), buf[(n + 1) & 1].begin() + before);
  return ok;
}

// floats in value order as unsigned keys (for the bisection below)
uint32_t key_of(float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
float float_of(uint32_t k) {
  const uint32_t b = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}
}  // namespace

// The smallest float x in [-1, 1] with get_angle(x) < T, found by bisection on the float's bits; exact
// when acosf is monotonic on [-1, 1], and verified at the result and at its predecessor, so a wrong
// threshold is an error, never a result.
DotThreshold angle_dot_threshold(float T, float& D) {
  auto pass = [T](float x) { return get_angle(x) < T; };
  if (!pass(1.0f)) return DotThreshold::kNonePasses;
  if (pass(-1.0f)) { D = -1.0f; return DotThreshold::kOk; }
  uint32_t lo = key_of(-1.0f), hi = key_of(1.0f);   // pass(lo) false, pass(hi) true
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (pass(float_of(mid))) hi = mid; else lo = mid;
  }
  D = float_of(hi);
  const float prev = std::nextafter(D, -2.0f);
  return get_angle(D) < T && T <= get_angle(prev) ? DotThreshold::kOk : DotThreshold::kUnverified;
}

// D[k], k = 2..n-1: angle_dot_threshold of the Intermediate angle threshold at k
bool tat_thresholds(float* D, int n, std::string& err) {
  for (int k = 0; k < n && k < 2; ++k) D[k] = 0.0f;
  for (int k = 2; k < n; ++k) {
    const DotThreshold r = angle_dot_threshold(angle_threshold(k), D[k]);
    if (r == DotThreshold::kNonePasses) { err = "fusion: no dot product passes the angle test at k = " + std::to_string(k); return false; }
    if (r == DotThreshold::kUnverified) {
      err = "fusion: the angle threshold table does not verify at k = " + std::to_string(k);
      return false;
    }
  }
  return true;
}

bool run_fusion_tat(std::vector<FusionView>& views, int mode, DpeContext* ctx, std::vector<FusedPoint>& cloud,
                    std::string& err) {
  if (mode != DPE_FUSION_TAT_INTERMEDIATE && mode != DPE_FUSION_TAT_ADVANCED) { err = "fusion: bad mode"; return false; }
  const Plan pl = fusion_plan(views);
  for (const auto& s : pl.srcs)
    if (s.size() > 31) { err = "fusion: more than 31 source views"; return false; }
  for (FusionView& v : views) v.mask.assign((size_t)v.view.width * v.view.height, 0);
  if (ctx && !pl.aliased) return tat_device(views, pl, mode, ctx, cloud, err);
  if (mode == DPE_FUSION_TAT_INTERMEDIATE) tat_intermediate_serial(views, pl, cloud);
  else tat_advanced_serial(views, pl, cloud);
  return true;
}

}  // namespace dpe_host

extern "C" {

long long dpe_host_fusion_tat_serial(int mode, const DpeHostTatView* views, int n, DpeFusedPoint* out, size_t cap) {
  return dpe_host_fusion_tat_run(mode, views, n, -1, out, cap);
}

long long dpe_host_fusion_tat_run(int mode, const DpeHostTatView* views, int n, int gpu_index, DpeFusedPoint* out,
                                  size_t cap) {
  if (!views || n < 1 || (!out && cap > 0)) return -1;
  std::vector<dpe_host::FusionView> fv(n);
  for (int i = 0; i < n; ++i) {
    const DpeHostTatView& v = views[i];
    if (v.view.width < 1 || v.view.height < 1 || !v.view.depth || !v.view.normal || !v.bgr || v.n_src < 0 ||
        (v.n_src > 0 && !v.src_ids))
      return -1;
    const size_t L = (size_t)v.view.width * v.view.height;
    fv[i].image_id = v.image_id;
    fv[i].src_ids.assign(v.src_ids, v.src_ids + v.n_src);
    fv[i].view = v.view;
    fv[i].bgr.assign(v.bgr, v.bgr + 3 * L);
    if (v.block) fv[i].block.assign(v.block, v.block + L);
  }
  std::vector<dpe_host::FusedPoint> cloud;
  std::string err;
  DpeContext* ctx = gpu_index >= 0 ? dpe_create(gpu_index) : nullptr;
  if (gpu_index >= 0 && !ctx) return -1;
  const bool ok = dpe_host::run_fusion_tat(fv, mode, ctx, cloud, err);
  if (ctx) dpe_destroy(ctx);
  if (!ok) return -1;
  for (int i = 0; i < n; ++i)
    if (views[i].mask) std::memcpy(views[i].mask, fv[i].mask.data(), fv[i].mask.size());
  if (!cloud.empty()) std::memcpy(out, cloud.data(), std::min(cap, cloud.size()) * sizeof(DpeFusedPoint));
  return (long long)cloud.size();
}

int dpe_host_fusion_tat_thresholds(float* D, int n) {
  std::string err;
  if (!D || n < 0) return 1;
  return dpe_host::tat_thresholds(D, n, err) ? 0 : 1;
}

int dpe_host_fusion_tat_angle_test(float dot, int k) {
  return dpe_host::get_angle(dot) < dpe_host::angle_threshold(k) ? 1 : 0;
}

}  // extern "C"
