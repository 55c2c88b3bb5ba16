// dpe_state.hip -- the resident states of include/dpe_mvs.h (dpe_state_save / fetch / snapshot /
// export_depth / import_depth / clear), the pass's device-side outputs (dpe_pm_device_planes,
// dpe_pm_export_depth), the exchange buffers, dpe_sync, dpe_device_copy and host pinning.  A unit of
// libdpe_mvs.so; the context and the concurrency contract are dpe_mvs.hip's (dpe_entry.h).
#include <hip/hip_runtime.h>
#include <string>
#include <vector>

#include "dpe_entry.h"
#include "dpe_context.h"

using namespace dpe;

extern "C" void* dpe_pm_device_planes(DpeContext* c) { return (c && c->pass.staged) ? (void*)c->pass.bufs.planes : nullptr; }

__global__ void k_export_depth(const float4* __restrict__ p, float* __restrict__ d, size_t L) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < L) d[i] = p[i].w;
}

extern "C" int dpe_pm_export_depth(DpeContext* c, float* dev_dst, void* stream_) {
  TRY(enter(c, dev_dst != nullptr, "dpe_pm_export_depth: null argument"));
  if (!c->pass.staged) { g_err = "dpe_pm_export_depth: nothing staged"; return DPE_ERR_STATE; }
  hipStream_t s;
  HIPC(enqueue_stream(c, stream_, &s));   // after the pass that writes the planes
  const size_t L = (size_t)c->pass.hc.W * c->pass.hc.H;
  k_export_depth<<<(unsigned)((L + 255) / 256), 256, 0, s>>>(c->pass.bufs.planes, dev_dst, L);
  HIPC(hipGetLastError());
  return DPE_OK;
}

// ------------------------------------------------------------------------------ resident state
// ProcessProblem's epilogue (main.cpp:423-437) on the pass outputs, into the image's resident state
__global__ void k_state_save(const float4* __restrict__ planes, const uint8_t* __restrict__ weak,
                             const uint32_t* __restrict__ sel, float dmin, float dmax, float4* __restrict__ op,
                             uint8_t* __restrict__ ow, uint32_t* __restrict__ os, size_t L) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L) return;
  float4 p = planes[i];
  uint8_t w = weak[i];
  if (p.w < dmin || p.w > dmax) { p.w = 0.0f; w = DPE_UNKNOWN; }
  op[i] = p; ow[i] = w; os[i] = sel[i];
}
__global__ void k_depth_of(const float4* __restrict__ p, float* __restrict__ d, size_t L) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < L) d[i] = p[i].w;
}
__global__ void k_depth_into(const float* __restrict__ d, float4* __restrict__ p, size_t L) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < L) p[i].w = d[i];
}

extern "C" int dpe_state_save(DpeContext* c, int image_id) {
  TRY(enter(c, true, "dpe_state_save: null context"));
  if (!c->pass.staged) { g_err = "dpe_state_save: nothing staged"; return DPE_ERR_STATE; }
  Range range_("dpe_state_save");
  const PassWork& pw = c->pass;
  const int W = pw.hc.W, H = pw.hc.H;
  const size_t L = (size_t)W * H;
  hipStream_t s;
  HIPC(enqueue_stream(c, nullptr, &s));   // the context's stream, after the pass that wrote the outputs
  ResState* r = &c->rstore[image_id];
  HIPC(r->planes.ensure(L)); HIPC(r->weak.ensure(L)); HIPC(r->sel.ensure(L));
  r->w = W; r->h = H; r->full = true;
  k_state_save<<<(unsigned)((L + 255) / 256), 256, 0, s>>>(pw.bufs.planes, pw.bufs.weak, pw.bufs.sel, pw.hc.P.depth_min,
                                                          pw.hc.P.depth_max, r->planes.p, r->weak.p, r->sel.p, L);
  HIPC(hipGetLastError());
  HIPC(mark_pending(c, s));   // the next execute / stage waits for the save too
  return DPE_OK;
}

extern "C" int dpe_state_fetch(DpeContext* c, int image_id, int* w, int* h, float* depth, float* normal, uint8_t* weak,
                               uint32_t* sel) {
  TRY(enter(c, true, "dpe_state_fetch: null context"));
  auto it = c->rstore.find(image_id);
  if (it == c->rstore.end()) { g_err = "dpe_state_fetch: no state of image " + std::to_string(image_id); return DPE_ERR_STATE; }
  const ResState* r = &it->second;
  if (w) *w = r->w;
  if (h) *h = r->h;
  const size_t L = (size_t)r->w * r->h;
  HIPC(host_wait(c));
  if (depth || normal) {
    std::vector<float4> p(L);
    HIPC(hipMemcpy(p.data(), r->planes.p, L * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < L; ++i) {
      if (depth) depth[i] = p[i].w;
      if (normal) { normal[3 * i] = p[i].x; normal[3 * i + 1] = p[i].y; normal[3 * i + 2] = p[i].z; }
    }
  }
  if (weak || sel) {
    if (!r->full) { g_err = "dpe_state_fetch: image " + std::to_string(image_id) + " holds a depth map only"; return DPE_ERR_STATE; }
    if (weak) HIPC(hipMemcpy(weak, r->weak.p, L, hipMemcpyDeviceToHost));
    if (sel) HIPC(hipMemcpy(sel, r->sel.p, L * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  return DPE_OK;
}

extern "C" int dpe_state_snapshot(DpeContext* c) {
  TRY(enter(c, true, "dpe_state_snapshot: null context"));
  hipStream_t s;
  HIPC(enqueue_stream(c, nullptr, &s));
  for (auto& kv : c->rstore) {
    ResState* r = &kv.second;
    const size_t L = (size_t)r->w * r->h;
    HIPC(r->snap.ensure(L));
    k_depth_of<<<(unsigned)((L + 255) / 256), 256, 0, s>>>(r->planes.p, r->snap.p, L);
    r->snap_w = r->w; r->snap_h = r->h;
    r->has_snap = true;
  }
  HIPC(hipGetLastError());
  HIPC(mark_pending(c, s));
  c->snap_mode = true;
  return DPE_OK;
}

extern "C" int dpe_state_export_depth(DpeContext* c, int image_id, float* dev_dst, void* stream_) {
  TRY(enter(c, dev_dst != nullptr, "dpe_state_export_depth: null argument"));
  auto it = c->rstore.find(image_id);
  if (it == c->rstore.end()) { g_err = "dpe_state_export_depth: no state of image " + std::to_string(image_id); return DPE_ERR_STATE; }
  hipStream_t s;
  HIPC(enqueue_stream(c, stream_, &s));
  const size_t L = (size_t)it->second.w * it->second.h;
  k_depth_of<<<(unsigned)((L + 255) / 256), 256, 0, s>>>(it->second.planes.p, dev_dst, L);
  HIPC(hipGetLastError());
  return DPE_OK;
}

extern "C" int dpe_state_import_depth(DpeContext* c, int image_id, int w, int h, const float* dev_src, void* stream_) {
  TRY(enter(c, dev_src && w > 0 && h > 0, "dpe_state_import_depth: bad argument"));
  hipStream_t s;
  HIPC(enqueue_stream(c, stream_, &s));   // an execute may still read this state's depth
  ResState* r = &c->rstore[image_id];
  const size_t L = (size_t)w * h;
  if (r->w != w || r->h != h) {
    HIPC(r->planes.ensure(L));
    HIPC(hipMemsetAsync(r->planes.p, 0, L * sizeof(float4), s));
    r->w = w; r->h = h; r->full = false;
  }
  k_depth_into<<<(unsigned)((L + 255) / 256), 256, 0, s>>>(dev_src, r->planes.p, L);
  HIPC(hipGetLastError());
  HIPC(publish_foreign(c, s));   // later stages on the context stream read it
  return DPE_OK;
}

extern "C" void dpe_state_clear(DpeContext* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)host_wait(c);
  c->rstore.clear();
  c->snap_mode = false;
#if DPE_GN_ONCE
  c->pass.gn_done_for_stage = false;
#endif
}

extern "C" float* dpe_device_buffer(DpeContext* c, int slot, size_t count) {
  g_err.clear();
  if (!c || slot < 0 || slot > 1) { g_err = "dpe_device_buffer: bad argument"; return nullptr; }
  if (hipSetDevice(c->device) != hipSuccess) { g_err = "dpe_device_buffer: hipSetDevice"; return nullptr; }
  if (c->xbuf[slot].n < count) {
    if (host_wait(c) != hipSuccess) { g_err = "dpe_device_buffer: sync"; return nullptr; }
    if (c->xbuf[slot].ensure(count) != hipSuccess) { g_err = "dpe_device_buffer: hipMalloc"; return nullptr; }
  }
  return c->xbuf[slot].p;
}

extern "C" int dpe_sync(DpeContext* c) {
  TRY(enter(c, true, "dpe_sync: null context"));
  HIPC(host_wait(c));
  return DPE_OK;
}

extern "C" int dpe_device_copy(DpeContext* c, void* dst, const void* src, size_t bytes, int kind) {
  TRY(enter(c, dst && src && kind >= 0 && kind <= 2, "dpe_device_copy: bad argument"));
  HIPC(host_wait(c));
  const hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice : (kind == 1 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice);
  HIPC(hipMemcpy(dst, src, bytes, k));
  return DPE_OK;
}

extern "C" int dpe_host_pin(void* ptr, size_t bytes) {
  if (!ptr || bytes == 0) return DPE_ERR_ARG;
  return hipHostRegister(ptr, bytes, hipHostRegisterDefault) == hipSuccess ? DPE_OK : DPE_ERR_HIP;
}
extern "C" int dpe_host_unpin(void* ptr) {
  if (!ptr) return DPE_ERR_ARG;
  return hipHostUnregister(ptr) == hipSuccess ? DPE_OK : DPE_ERR_HIP;
}
