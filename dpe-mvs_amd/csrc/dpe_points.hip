// dpe_points.hip -- the per-image point clouds of include/dpe_mvs.h (dpe_state_point_cloud*,
// dpe_point_cloud_arrays): the kernels of pass_points.h over the resident states and the context's
// points scratch.  A unit of libdpe_mvs.so; the concurrency contract is dpe_mvs.hip's (dpe_entry.h).
#include <hip/hip_runtime.h>
#include <atomic>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "pass_points.h"
#include "dpe_entry.h"
#include "dpe_context.h"

using namespace dpe;

static_assert(sizeof(TatPoint) == sizeof(DpeFusedPoint), "the kernels write DpeFusedPoint records");

static std::atomic<long long> g_points_launches{0};

extern "C" long long dpe_points_launches(void) { return g_points_launches.load(); }

static bool points_mode_ok(int mode) { return mode == DPE_POINTS_ALL || mode == DPE_POINTS_STRONG; }

// Count, scan and fill of (planes, weak, c->points.bgr) into c->points.out on stream s, then the host
// waits for the total: *n.  More than `cap` points: DPE_ERR_ARG.  The n points are copied into `out`
// on s (asynchronously when `out` is pinned).
static int points_run(DpeContext* c, int mode, const float4* planes, const uint8_t* weak, const DpeCamera& cam, int w, int h,
                      float dmin, float dmax, DpeFusedPoint* out, size_t cap, size_t* n, hipStream_t s, const char* who) {
  PointsScratch& v = c->points;
  const size_t L = (size_t)w * h;
  const int nseg = (h + kPtsSeg - 1) / kPtsSeg;
  const size_t ncell = (size_t)w * nseg;
  HIPC(v.cnt.ensure(ncell));
  HIPC(v.tot.ensure(1));
  HIPC(v.out.ensure(L));
  const dim3 grid((unsigned)((w + kPtsCols - 1) / kPtsCols), (unsigned)nseg);
  k_pts_count<<<grid, kPtsCols, 0, s>>>(mode, planes, weak, w, h, nseg, dmin, dmax, v.cnt.p);
  HIPC(hipGetLastError());
  k_offsets_scan<256><<<1, 256, 0, s>>>((int)ncell, v.cnt.p, v.tot.p);
  HIPC(hipGetLastError());
  k_pts_fill<<<grid, kPtsCols, 0, s>>>(mode, planes, weak, v.bgr.p, cam, w, h, nseg, dmin, dmax, v.cnt.p, v.out.p);
  HIPC(hipGetLastError());
  g_points_launches += 3;
  int total = 0;
  HIPC(hipMemcpyAsync(&total, v.tot.p, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  *n = (size_t)total;
  if ((size_t)total > cap) { g_err = std::string(who) + ": point buffer too small"; return DPE_ERR_ARG; }
  if (total > 0) HIPC(hipMemcpyAsync(out, v.out.p, (size_t)total * sizeof(DpeFusedPoint), hipMemcpyDeviceToHost, s));
  return DPE_OK;
}

// the limits of the kernels' int indices: cells, points and grid rows
static bool points_size_ok(int w, int h) {
  return w >= 1 && h >= 1 && (size_t)w * h < (size_t)1 << 31 && (size_t)w * ((h + kPtsSeg - 1) / kPtsSeg) < (size_t)1 << 31 &&
         (h + kPtsSeg - 1) / kPtsSeg <= 65535;
}

extern "C" int dpe_state_point_cloud(DpeContext* c, int image_id, int mode, const DpeCamera* cam, const uint8_t* host_bgr,
                                     float dmin, float dmax, DpeFusedPoint* out, size_t cap, size_t* n, void* stream_) {
  TRY(enter(c, cam && host_bgr && n && (out || cap == 0), "dpe_state_point_cloud: null argument"));
  *n = 0;
  if (!points_mode_ok(mode)) { g_err = "dpe_state_point_cloud: bad mode"; return DPE_ERR_ARG; }
  auto it = c->rstore.find(image_id);
  if (it == c->rstore.end()) { g_err = "dpe_state_point_cloud: no state of image " + std::to_string(image_id); return DPE_ERR_STATE; }
  const ResState& r = it->second;
  if (mode == DPE_POINTS_STRONG && !r.full) {
    g_err = "dpe_state_point_cloud: image " + std::to_string(image_id) + " holds a depth map only";
    return DPE_ERR_STATE;
  }
  if (!points_size_ok(r.w, r.h)) { g_err = "dpe_state_point_cloud: state too large"; return DPE_ERR_ARG; }
  hipStream_t s;
  HIPC(enqueue_stream(c, stream_, &s));   // after the save that wrote the state
  const size_t L = (size_t)r.w * r.h;
  HIPC(c->points.bgr.ensure(3 * L));
  HIPC(hipMemcpyAsync(c->points.bgr.p, host_bgr, 3 * L, hipMemcpyHostToDevice, s));
  TRY(points_run(c, mode, r.planes.p, r.weak.p, *cam, r.w, r.h, dmin, dmax, out, cap, n, s, "dpe_state_point_cloud"));
  hipEvent_t ev = nullptr;
  {
    std::lock_guard<std::mutex> lk(c->points.mu);
    auto e = c->points.ev.find(out);
    if (e == c->points.ev.end()) {
      Event fresh;
      HIPC(fresh.create());
      e = c->points.ev.emplace(out, std::move(fresh)).first;
    }
    ev = e->second;
  }
  HIPC(hipEventRecord(ev, s));
  HIPC(publish_foreign(c, s));   // the scratch is reused, and the state rewritten, by later work of the context
  return DPE_OK;
}

extern "C" int dpe_state_point_cloud_wait(DpeContext* c, const DpeFusedPoint* out) {
  g_err.clear();   // (not enter(): the lookup comes before the device is selected, and any host thread may call)
  if (!c) { g_err = "dpe_state_point_cloud_wait: null argument"; return DPE_ERR_ARG; }
  hipEvent_t ev = nullptr;
  {
    std::lock_guard<std::mutex> lk(c->points.mu);
    auto it = c->points.ev.find(out);
    if (it == c->points.ev.end()) { g_err = "dpe_state_point_cloud_wait: no point cloud into this buffer"; return DPE_ERR_ARG; }
    ev = it->second;
  }
  HIPC(hipSetDevice(c->device));
  HIPC(hipEventSynchronize(ev));
  return DPE_OK;
}

extern "C" int dpe_point_cloud_arrays(DpeContext* c, int mode, int w, int h, const float* depth, const uint8_t* weak,
                                      const DpeCamera* cam, const uint8_t* bgr, float dmin, float dmax, DpeFusedPoint* out,
                                      size_t cap, size_t* n) {
  TRY(enter(c, depth && cam && bgr && n && (out || cap == 0) && points_size_ok(w, h), "dpe_point_cloud_arrays: bad argument"));
  *n = 0;
  if (!points_mode_ok(mode) || (mode == DPE_POINTS_STRONG && !weak)) {
    g_err = "dpe_point_cloud_arrays: bad mode or missing array";
    return DPE_ERR_ARG;
  }
  const size_t L = (size_t)w * h;
  std::vector<float4> p(L);
  for (size_t i = 0; i < L; ++i) p[i] = make_float4(0.f, 0.f, 0.f, depth[i]);
  HIPC(host_wait(c));
  PointsScratch& v = c->points;
  HIPC(v.planes.ensure(L));
  HIPC(v.weak.ensure(L));
  HIPC(v.bgr.ensure(3 * L));
  HIPC(hipMemcpy(v.planes.p, p.data(), L * sizeof(float4), hipMemcpyHostToDevice));
  if (weak) HIPC(hipMemcpy(v.weak.p, weak, L, hipMemcpyHostToDevice));
  else HIPC(hipMemset(v.weak.p, 0, L));
  HIPC(hipMemcpy(v.bgr.p, bgr, 3 * L, hipMemcpyHostToDevice));
  TRY(points_run(c, mode, v.planes.p, v.weak.p, *cam, w, h, dmin, dmax, out, cap, n, c->stream, "dpe_point_cloud_arrays"));
  HIPC(hipStreamSynchronize(c->stream));
  return DPE_OK;
}
