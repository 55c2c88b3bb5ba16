// dpe_viz.hip -- the viz medium results of include/dpe_mvs.h (dpe_state_render*, dpe_viz_render_arrays,
// dpe_jpeg_blocks_device): the kernels of pass_viz.h over the resident states and the context's viz
// scratch.  A unit of libdpe_mvs.so; the concurrency contract is dpe_mvs.hip's (dpe_entry.h).
#include <hip/hip_runtime.h>
#include <atomic>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "pass_viz.h"
#include "dpe_entry.h"
#include "dpe_context.h"

using namespace dpe;

static std::atomic<long long> g_viz_launches{0};

extern "C" long long dpe_viz_launches(void) { return g_viz_launches.load(); }

static size_t viz_block_values(int w, int h) { return (size_t)((w + 15) / 16) * ((h + 15) / 16) * 6 * 64; }

// the picture of (planes, weak) into c->viz.bgr on stream s
static int viz_enqueue_render(DpeContext* c, int kind, const float4* planes, const uint8_t* weak, int w, int h, float dmin,
                              float dmax, hipStream_t s) {
  const size_t L = (size_t)w * h;
  HIPC(c->viz.bgr.ensure(3 * L));
  k_viz_render<<<(unsigned)((L + 1023) / 1024), 256, 0, s>>>(kind, planes, weak, dmin, dmax, c->viz.bgr.p, L);
  HIPC(hipGetLastError());
  g_viz_launches++;
  return DPE_OK;
}

// the JPEG front half of c->viz.bgr (w x h) into c->viz.blocks on stream s
static int viz_enqueue_front(DpeContext* c, int w, int h, int quality, hipStream_t s) {
  VizScratch& v = c->viz;
  if (v.quality != quality) {   // first use, or another quality: no kernel may still read the old tables
    HIPC(hipStreamSynchronize(s));
    HIPC(hipStreamSynchronize(c->stream));
    uint16_t q[128];
    dpe_jpeg::quant_tables(quality, q);
    HIPC(v.q.ensure(128));
    HIPC(hipMemcpy(v.q.p, q, sizeof(q), hipMemcpyHostToDevice));
    v.quality = quality;
  }
  HIPC(v.blocks.ensure(viz_block_values(w, h)));
  k_jpeg_front<<<dim3((unsigned)((w + 15) / 16), (unsigned)((h + 15) / 16)), 384, 0, s>>>(v.bgr.p, w, h, v.q.p, v.blocks.p);
  HIPC(hipGetLastError());
  g_viz_launches++;
  return DPE_OK;
}

static const ResState* viz_state(DpeContext* c, int image_id, int kind, const char* who) {
  if (kind != DPE_VIZ_DEPTH && kind != DPE_VIZ_NORMAL && kind != DPE_VIZ_WEAK) { g_err = std::string(who) + ": bad kind"; return nullptr; }
  auto it = c->rstore.find(image_id);
  if (it == c->rstore.end()) { g_err = std::string(who) + ": no state of image " + std::to_string(image_id); return nullptr; }
  if (!it->second.full) { g_err = std::string(who) + ": image " + std::to_string(image_id) + " holds a depth map only"; return nullptr; }
  return &it->second;
}

extern "C" int dpe_state_render(DpeContext* c, int image_id, int kind, float dmin, float dmax, uint8_t* host_bgr) {
  TRY(enter(c, host_bgr != nullptr, "dpe_state_render: null argument"));
  const ResState* r = viz_state(c, image_id, kind, "dpe_state_render");
  if (!r) return g_err.find("bad kind") != std::string::npos ? DPE_ERR_ARG : DPE_ERR_STATE;
  hipStream_t s;
  HIPC(enqueue_stream(c, nullptr, &s));
  TRY(viz_enqueue_render(c, kind, r->planes.p, r->weak.p, r->w, r->h, dmin, dmax, s));
  HIPC(hipMemcpyAsync(host_bgr, c->viz.bgr.p, (size_t)r->w * r->h * 3, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  return DPE_OK;
}

extern "C" int dpe_state_render_jpeg_blocks(DpeContext* c, int image_id, int kind, float dmin, float dmax, int quality,
                                            int16_t* host_blocks, size_t cap, void* stream_) {
  TRY(enter(c, host_blocks != nullptr, "dpe_state_render_jpeg_blocks: null argument"));
  if (quality < 1 || quality > 100) { g_err = "dpe_state_render_jpeg_blocks: bad quality"; return DPE_ERR_ARG; }
  const ResState* r = viz_state(c, image_id, kind, "dpe_state_render_jpeg_blocks");
  if (!r) return g_err.find("bad kind") != std::string::npos ? DPE_ERR_ARG : DPE_ERR_STATE;
  const size_t n = viz_block_values(r->w, r->h);
  if (cap < n) { g_err = "dpe_state_render_jpeg_blocks: block buffer too small"; return DPE_ERR_ARG; }
  hipStream_t s;
  HIPC(enqueue_stream(c, stream_, &s));   // after the save that wrote the state
  TRY(viz_enqueue_render(c, kind, r->planes.p, r->weak.p, r->w, r->h, dmin, dmax, s));
  TRY(viz_enqueue_front(c, r->w, r->h, quality, s));
  HIPC(hipMemcpyAsync(host_blocks, c->viz.blocks.p, n * sizeof(int16_t), hipMemcpyDeviceToHost, s));
  hipEvent_t ev = nullptr;
  {
    std::lock_guard<std::mutex> lk(c->viz.mu);
    auto it = c->viz.ev.find(host_blocks);
    if (it == c->viz.ev.end()) {
      Event fresh;
      HIPC(fresh.create());
      it = c->viz.ev.emplace(host_blocks, std::move(fresh)).first;
    }
    ev = it->second;
  }
  HIPC(hipEventRecord(ev, s));
  HIPC(publish_foreign(c, s));   // the scratch is reused, and the state rewritten, by later work of the context
  return DPE_OK;
}

extern "C" int dpe_state_render_wait(DpeContext* c, const int16_t* host_blocks) {
  g_err.clear();   // (not enter(): the lookup comes before the device is selected, and any host thread may call)
  if (!c || !host_blocks) { g_err = "dpe_state_render_wait: null argument"; return DPE_ERR_ARG; }
  hipEvent_t ev = nullptr;
  {
    std::lock_guard<std::mutex> lk(c->viz.mu);
    auto it = c->viz.ev.find(host_blocks);
    if (it == c->viz.ev.end()) { g_err = "dpe_state_render_wait: no render into this buffer"; return DPE_ERR_ARG; }
    ev = it->second;
  }
  HIPC(hipSetDevice(c->device));
  HIPC(hipEventSynchronize(ev));
  return DPE_OK;
}

extern "C" int dpe_viz_render_arrays(DpeContext* c, int kind, int w, int h, const float* depth, const float* normal,
                                     const uint8_t* weak, float dmin, float dmax, uint8_t* host_bgr) {
  TRY(enter(c, host_bgr && w >= 1 && h >= 1, "dpe_viz_render_arrays: bad argument"));
  if (kind == DPE_VIZ_DEPTH ? !depth : kind == DPE_VIZ_NORMAL ? !normal : kind == DPE_VIZ_WEAK ? !weak : true) {
    g_err = "dpe_viz_render_arrays: bad kind or missing array";
    return DPE_ERR_ARG;
  }
  const size_t L = (size_t)w * h;
  std::vector<float4> p(L);
  for (size_t i = 0; i < L; ++i)
    p[i] = make_float4(normal ? normal[3 * i] : 0.f, normal ? normal[3 * i + 1] : 0.f, normal ? normal[3 * i + 2] : 0.f,
                       depth ? depth[i] : 0.f);
  HIPC(host_wait(c));
  VizScratch& v = c->viz;
  HIPC(v.planes.ensure(L));
  HIPC(v.weak.ensure(L));
  HIPC(hipMemcpy(v.planes.p, p.data(), L * sizeof(float4), hipMemcpyHostToDevice));
  if (weak) HIPC(hipMemcpy(v.weak.p, weak, L, hipMemcpyHostToDevice));
  else HIPC(hipMemset(v.weak.p, 0, L));
  TRY(viz_enqueue_render(c, kind, v.planes.p, v.weak.p, w, h, dmin, dmax, c->stream));
  HIPC(hipMemcpyAsync(host_bgr, v.bgr.p, 3 * L, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  return DPE_OK;
}

extern "C" int dpe_jpeg_blocks_device(DpeContext* c, const uint8_t* host_bgr, int w, int h, int quality, int16_t* host_blocks,
                                      size_t cap) {
  TRY(enter(c, host_bgr && host_blocks && w >= 1 && h >= 1 && w <= 65535 && h <= 65535 && quality >= 1 && quality <= 100,
            "dpe_jpeg_blocks_device: bad argument"));
  const size_t n = viz_block_values(w, h);
  if (cap < n) { g_err = "dpe_jpeg_blocks_device: block buffer too small"; return DPE_ERR_ARG; }
  HIPC(host_wait(c));
  HIPC(c->viz.bgr.ensure((size_t)w * h * 3));
  HIPC(hipMemcpy(c->viz.bgr.p, host_bgr, (size_t)w * h * 3, hipMemcpyHostToDevice));
  TRY(viz_enqueue_front(c, w, h, quality, c->stream));
  HIPC(hipMemcpyAsync(host_blocks, c->viz.blocks.p, n * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  return DPE_OK;
}
