// dpe_fusion.hip -- the fusions of include/dpe_mvs.h on the GPU: dpe_fusion_stage and
// dpe_fusion_candidates (pass_fusion.h), and the two Tanks-and-Temples fusions dpe_fusion_tat_*
// (pass_fusion_tat.h) and the consistency maps dpe_fusion_consistency (pass_consistency.h) over the
// staged views.  A unit of libdpe_mvs.so.  The calls use the context's
// stream and synchronise it before they return; the one copy dpe_fusion_tat_image leaves in flight
// is described with the concurrency contract in dpe_mvs.hip.
#include <hip/hip_runtime.h>
#include <atomic>
#include <string>
#include <vector>

#include "pass_fusion.h"
#include "pass_fusion_tat.h"
#include "pass_consistency.h"
#include "dpe_entry.h"
#include "dpe_context.h"

using namespace dpe;

extern "C" int dpe_fusion_stage(DpeContext* c, const DpeFusionView* views, int n) {
  TRY(enter(c, views && n >= 1, "dpe_fusion_stage: bad argument"));
  c->tat.views_restaged();
  FusionStage& fz = c->fz;
  fz.depth.resize(n); fz.normal.resize(n); fz.host.assign(n, FusionViewDev{});
  std::vector<DpeCamera> cams(n);
  for (int i = 0; i < n; ++i) {
    const DpeFusionView& v = views[i];
    if (v.width < 1 || v.height < 1 || !v.depth || !v.normal) { g_err = "dpe_fusion_stage: bad view"; return DPE_ERR_ARG; }
    const size_t L = (size_t)v.width * v.height;
    HIPC(fz.depth[i].ensure(L));
    HIPC(fz.normal[i].ensure(3 * L));
    HIPC(hipMemcpyAsync(fz.depth[i].p, v.depth, L * 4, hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(fz.normal[i].p, v.normal, 3 * L * 4, hipMemcpyHostToDevice, c->stream));
    fz.host[i] = FusionViewDev{fz.depth[i].p, fz.normal[i].p, v.width, v.height};
    cams[i] = v.cam;
  }
  HIPC(fz.views.ensure(n));
  HIPC(fz.cams.ensure(n));
  HIPC(hipMemcpyAsync(fz.views.p, fz.host.data(), n * sizeof(FusionViewDev), hipMemcpyHostToDevice, c->stream));
  HIPC(hipMemcpyAsync(fz.cams.p, cams.data(), n * sizeof(DpeCamera), hipMemcpyHostToDevice, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  fz.n = n;
  return DPE_OK;
}

// What the entries over the staged views refuse, in this order and with the entry's name in front: nothing staged,
// a reference view outside them, a source view outside them and (unless self_ok) the reference view among its sources
static int views_check(DpeContext* c, const char* who, int ref, const int* src, int ns, bool self_ok) {
  const int n = c->fz.n;
  if (n < 1) { g_err = std::string(who) + ": nothing staged"; return DPE_ERR_STATE; }
  if (ref < 0 || ref >= n) { g_err = std::string(who) + ": bad reference view"; return DPE_ERR_ARG; }
  for (int j = 0; j < ns; ++j) {
    if (src[j] < 0 || src[j] >= n) { g_err = std::string(who) + ": bad source view"; return DPE_ERR_ARG; }
    if (!self_ok && src[j] == ref) { g_err = std::string(who) + ": the reference view is among its sources"; return DPE_ERR_ARG; }
  }
  return DPE_OK;
}

extern "C" int dpe_fusion_candidates(DpeContext* c, int ref, const int* src, int ns, int32_t* idx, float* val) {
  TRY(enter(c, src && idx && val && ns >= 0, "dpe_fusion_candidates: bad argument"));
  FusionStage& fz = c->fz;
  TRY(views_check(c, "dpe_fusion_candidates", ref, src, ns, true));   // a view may be among its own sources here
  if (ns == 0) return DPE_OK;
  const size_t L = (size_t)fz.host[ref].w * fz.host[ref].h;
  HIPC(fz.src.ensure(ns));
  HIPC(fz.idx.ensure(L * ns));
  HIPC(fz.val.ensure(L * ns * 3));
  HIPC(hipMemcpyAsync(fz.src.p, src, ns * sizeof(int), hipMemcpyHostToDevice, c->stream));
  k_fusion_candidates<<<(unsigned)((L + 255) / 256), 256, 0, c->stream>>>(fz.cams.p, fz.views.p, ref, fz.src.p, ns, fz.idx.p,
                                                                         fz.val.p);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(idx, fz.idx.p, L * ns * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPC(hipMemcpyAsync(val, fz.val.p, L * ns * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  return DPE_OK;
}

static std::atomic<long long> g_consistency_launches{0};

extern "C" long long dpe_consistency_launches(void) { return g_consistency_launches.load(); }

extern "C" int dpe_fusion_consistency(DpeContext* c, int ref, const int* src, int ns, float dot_threshold, int min_views,
                                      uint8_t* count, float* depth_filtered) {
  TRY(enter(c, ns >= 0 && (ns == 0 || src), "dpe_fusion_consistency: bad argument"));
  if (ns > kConsistencyMaxSrc) { g_err = "dpe_fusion_consistency: more than 255 source views"; return DPE_ERR_ARG; }
  if (min_views < 1 || min_views > 255) { g_err = "dpe_fusion_consistency: min_views outside 1..255"; return DPE_ERR_ARG; }
  FusionStage& fz = c->fz;
  TRY(views_check(c, "dpe_fusion_consistency", ref, src, ns, false));
  const size_t L = (size_t)fz.host[ref].w * fz.host[ref].h;
  if (L >= (size_t)1 << 31) { g_err = "dpe_fusion_consistency: view too large"; return DPE_ERR_ARG; }   // the kernel's int pixel index
  HIPC(host_wait(c));   // the buffers below may grow, and the results are read on the host
  HIPC(fz.src.ensure(ns > 0 ? ns : 1));
  HIPC(fz.cons_count.ensure(L));
  HIPC(fz.cons_depth.ensure(L));
  if (ns > 0) HIPC(hipMemcpyAsync(fz.src.p, src, ns * sizeof(int), hipMemcpyHostToDevice, c->stream));
  k_consistency<<<(unsigned)((L + 255) / 256), 256, 0, c->stream>>>(fz.cams.p, fz.views.p, ref, fz.src.p, ns, dot_threshold,
                                                                   min_views, fz.cons_count.p, fz.cons_depth.p);
  HIPC(hipGetLastError());
  g_consistency_launches += 1;
  if (count) HIPC(hipMemcpyAsync(count, fz.cons_count.p, L, hipMemcpyDeviceToHost, c->stream));
  if (depth_filtered) HIPC(hipMemcpyAsync(depth_filtered, fz.cons_depth.p, L * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));   // also before the caller's `src` goes out of scope
  return DPE_OK;
}

// host-waits for the copy-out of the last dpe_fusion_tat_image
static hipError_t tat_wait_copy(DpeContext* c) {
  hipError_t e = hipSuccess;
  if (c->tat.copying) { e = hipEventSynchronize(c->tat.ev); c->tat.copying = false; }
  return e;
}

extern "C" int dpe_fusion_tat_begin(DpeContext* c, const uint8_t* const* bgr, const uint8_t* const* block) {
  TRY(enter(c, bgr != nullptr, "dpe_fusion_tat_begin: bad argument"));
  if (c->fz.n < 1) { g_err = "dpe_fusion_tat_begin: nothing staged"; return DPE_ERR_STATE; }
  const int n = c->fz.n;
  for (int i = 0; i < n; ++i)
    if (!bgr[i]) { g_err = "dpe_fusion_tat_begin: missing colour image"; return DPE_ERR_ARG; }
  HIPC(host_wait(c));
  HIPC(tat_wait_copy(c));
  TatFusion& tat = c->tat;
  tat.ready = false;
  tat.bgr.resize(n); tat.block.resize(n); tat.mask.resize(n);
  std::vector<TatViewDev> tv(n);
  for (int i = 0; i < n; ++i) {
    const size_t L = (size_t)c->fz.host[i].w * c->fz.host[i].h;
    HIPC(tat.bgr[i].ensure(3 * L));
    HIPC(tat.mask[i].ensure(L));
    HIPC(hipMemcpyAsync(tat.bgr[i].p, bgr[i], 3 * L, hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemsetAsync(tat.mask[i].p, 0, L, c->stream));
    const bool blk = block && block[i];
    if (blk) {
      HIPC(tat.block[i].ensure(L));
      HIPC(hipMemcpyAsync(tat.block[i].p, block[i], L, hipMemcpyHostToDevice, c->stream));
    }
    tv[i] = TatViewDev{tat.bgr[i].p, blk ? tat.block[i].p : nullptr, tat.mask[i].p};
  }
  HIPC(tat.views.ensure(n));
  HIPC(hipMemcpyAsync(tat.views.p, tv.data(), n * sizeof(TatViewDev), hipMemcpyHostToDevice, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  tat.ready = true;
  return DPE_OK;
}

extern "C" int dpe_fusion_tat_image(DpeContext* c, int mode, int ref, const int* src, int ns, const float* dot_thresholds,
                                    DpeFusedPoint* out, size_t cap, size_t* n_out) {
  static_assert(sizeof(DpeFusedPoint) == sizeof(TatPoint), "DpeFusedPoint layout");
  TRY(enter(c, n_out && ns >= 0 && (ns == 0 || src) && (out || cap == 0), "dpe_fusion_tat_image: bad argument"));
  FusionStage& fz = c->fz;
  TatFusion& tat = c->tat;
  if (!tat.ready) { g_err = "dpe_fusion_tat_image: dpe_fusion_tat_begin has not run"; return DPE_ERR_STATE; }
  if (mode != DPE_FUSION_TAT_INTERMEDIATE && mode != DPE_FUSION_TAT_ADVANCED) { g_err = "dpe_fusion_tat_image: bad mode"; return DPE_ERR_ARG; }
  TRY(views_check(c, "dpe_fusion_tat_image", ref, nullptr, 0, true));   // the reference view before the limit, the sources after
  if (ns > kTatMaxSrc) { g_err = "dpe_fusion_tat_image: more than 31 source views"; return DPE_ERR_TOO_MANY; }
  // the kernels read the masks of the source views while they write the reference view's
  TRY(views_check(c, "dpe_fusion_tat_image", ref, src, ns, false));
  if (mode == DPE_FUSION_TAT_INTERMEDIATE && ns >= 2 && !dot_thresholds) { g_err = "dpe_fusion_tat_image: no thresholds"; return DPE_ERR_ARG; }
  *n_out = 0;
  if (ns < 2) {   // the k loop starts at 2 (DPE.cpp:1504): no point, no mask
    HIPC(tat_wait_copy(c));
    return DPE_OK;
  }
  const size_t L = (size_t)fz.host[ref].w * fz.host[ref].h;
  const int nch = (int)((L + kTatChunk - 1) / kTatChunk);
  DevArr<TatPoint>& dout = tat.out[tat.turn];
  HIPC(fz.src.ensure(ns));
  HIPC(tat.dthr.ensure(kTatMaxSrc + 1));
  HIPC(tat.last.ensure(L * ns));
  HIPC(tat.agg.ensure((size_t)nch * ns));
  HIPC(tat.cnt.ensure(nch));
  HIPC(tat.tot.ensure(1));
  HIPC(tat.emit.ensure(L));
  HIPC(tat.rec.ensure(L));
  HIPC(dout.ensure(L));
  hipStream_t s;
  HIPC(enqueue_stream(c, nullptr, &s));
  float dthr[kTatMaxSrc + 1] = {0};
  if (mode == DPE_FUSION_TAT_INTERMEDIATE)
    for (int k = 2; k <= ns; ++k) dthr[k] = dot_thresholds[k];
  // (the stream is synchronised below, before `dthr` and the caller's `src` go out of scope)
  HIPC(hipMemcpyAsync(fz.src.p, src, ns * sizeof(int), hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(tat.dthr.p, dthr, sizeof(dthr), hipMemcpyHostToDevice, s));
  k_tat_hit_scan<<<nch, kTatChunk, 0, s>>>(fz.cams.p, fz.views.p, tat.views.p, ref, fz.src.p, ns, nch, tat.last.p, tat.agg.p);
  k_tat_chunk_carry<<<ns, 256, 0, s>>>(nch, tat.agg.p);
  k_tat_decide<<<nch, kTatChunk, 0, s>>>(fz.cams.p, fz.views.p, tat.views.p, ref, fz.src.p, ns, nch, mode, tat.dthr.p,
                                        tat.last.p, tat.agg.p, tat.rec.p, tat.emit.p, tat.cnt.p);
  k_offsets_scan<256><<<1, 256, 0, s>>>(nch, tat.cnt.p, tat.tot.p);
  k_tat_fill<<<nch, kTatChunk, 0, s>>>((int)L, tat.emit.p, tat.rec.p, tat.cnt.p, dout.p);
  HIPC(hipGetLastError());
  int total = 0;
  HIPC(hipMemcpyAsync(&total, tat.tot.p, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  HIPC(tat_wait_copy(c));   // the copy-out of the image before ran beside these kernels
  if (total < 0 || (size_t)total > L) { g_err = "dpe_fusion_tat_image: bad point count"; return DPE_ERR_STATE; }
  *n_out = (size_t)total;
  if ((size_t)total > cap) { g_err = "dpe_fusion_tat_image: output buffer too small"; return DPE_ERR_ARG; }
  if (total > 0) {
    HIPC(hipMemcpyAsync(out, dout.p, (size_t)total * sizeof(TatPoint), hipMemcpyDeviceToHost, c->aux));
    HIPC(hipEventRecord(tat.ev, c->aux));
    tat.copying = true;
    tat.turn ^= 1;
  }
  return DPE_OK;
}

extern "C" int dpe_fusion_tat_wait(DpeContext* c) {
  TRY(enter(c, true, "dpe_fusion_tat_wait: null context"));
  HIPC(tat_wait_copy(c));
  return DPE_OK;
}

extern "C" int dpe_fusion_tat_mask(DpeContext* c, int view, uint8_t* mask) {
  TRY(enter(c, mask != nullptr, "dpe_fusion_tat_mask: bad argument"));
  if (!c->tat.ready) { g_err = "dpe_fusion_tat_mask: dpe_fusion_tat_begin has not run"; return DPE_ERR_STATE; }
  if (view < 0 || view >= c->fz.n) { g_err = "dpe_fusion_tat_mask: bad view"; return DPE_ERR_ARG; }
  HIPC(host_wait(c));
  HIPC(hipMemcpy(mask, c->tat.mask[view].p, (size_t)c->fz.host[view].w * c->fz.host[view].h, hipMemcpyDeviceToHost));
  return DPE_OK;
}
