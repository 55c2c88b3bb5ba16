// dpe_mvs.hip — the main unit of the C-ABI library (include/dpe_mvs.h): the context's life cycle,
// the entry-point rules every unit shares (dpe_entry.h: error string, prologue, waiting), HBM staging
// and the launch sequence of one PatchMatch pass on gfx950.  The other entry points are in units of
// their own: dpe_state.hip (resident states, exchange buffers), dpe_edges.hip (EdgeSegment stages),
// dpe_viz.hip (viz medium results) and dpe_fusion.hip (the fusions); the strong sweep, DepthToWeak
// and LocalRefine launch from tap_launch.hip / tap_f32.hip.
//
// Replaces DPE::CudaSpaceInitialization / SetDataPassHelperInCuda / RunPatchMatch / getters
// (DPE.cpp:916-1121, DPE.cu:3126-3249).  Differences by design:
//   * no per-launch cudaDeviceSynchronize: the 26 launches are queued on one stream;
//   * device buffers persist in the context across passes (resized only when W/H/N grow);
//   * the bilinear texture path is a padded quad-texel image in HBM (one 16-B load per tap);
//   * cuRAND states (48 B/px + curand_init) are replaced by counter-based Philox;
//   * errors are return codes (no exit()).
// dpe_pm_stage is stage_impl's named steps; dpe_pm_execute is the named steps of one pass ("one
// pass" below) over the pixel-list layout of pass_lists.h.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <memory>
#include <utility>
#include <vector>

#include "pass_tables.h"
#include "pass_kernels.h"
#include "pass_neighbours.h"
#include "pass_refine.h"
#include "pass_sweep.h"
#include "tap_launch.h"
#include "dpe_entry.h"
#include "dpe_context.h"

using namespace dpe;

static const int kDefaultXcdRows = 1;
static constexpr int kWeakLanes = 16;   // lanes per weak pixel in k_weak_coop

thread_local std::string dpe::g_err;

extern "C" {

void dpe_params_default(DpePatchMatchParams* p) {   // main.h:78-106
  p->max_iterations = 3;
  p->num_images = 5;
  p->sigma_spatial = 5.0f;
  p->sigma_color = 3.0f;
  p->top_k = 4;
  p->depth_min = 0.0f;
  p->depth_max = 1.0f;
  p->geom_consistency = false;
  p->strong_radius = 5;
  p->strong_increment = 2;
  p->weak_radius = 5;
  p->weak_increment = 5;
  p->use_APD = true;
  p->use_edge = true;
  p->use_limit = true;
  p->use_label = true;
  p->use_radius = true;
  p->high_res_img = true;
  p->max_scale_size = 1;
  p->scale_size = 1;
  p->weak_peak_radius = 2;
  p->rotate_time = 4;
  p->ransac_threshold = 0.005f;
  p->geom_factor = 0.2f;
  p->state = DPE_FIRST_INIT;
}

const char* dpe_last_error(void) { return g_err.c_str(); }

DpeContext* dpe_create(int device) {
  g_err.clear();
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) {
    g_err = "dpe_create: no such HIP device";
    return nullptr;
  }
  if (hipSetDevice(device) != hipSuccess) { g_err = "dpe_create: hipSetDevice failed"; return nullptr; }
  std::unique_ptr<DpeContext> c(new DpeContext());
  c->device = device;
  if (c->stream.create() != hipSuccess) { g_err = "dpe_create: stream"; return nullptr; }
  if (c->aux.create() != hipSuccess || c->ev_fork.create() != hipSuccess || c->ev_join.create() != hipSuccess ||
      c->ev_ei.create() != hipSuccess || c->ev_done.create() != hipSuccess || c->tat.ev.create() != hipSuccess ||
      c->ev_start.create(hipEventDefault) != hipSuccess) {
    g_err = "dpe_create: aux stream";
    return nullptr;
  }
  return c.release();
}

}  // extern "C"

// The concurrency contract of the entry points.  Work of the context runs on its own stream, or on
// the stream a caller passes; `ev_done` marks the end of the last work that may be on another stream
// than the context's, and `pending` says that nobody has waited for it yet.
//   * Entry points that read results on the host, overwrite or free buffers HOST-WAIT with
//     host_wait(): dpe_pm_fetch, dpe_state_fetch, dpe_state_clear, dpe_image_cache_clear, dpe_destroy,
//     dpe_sync, dpe_device_copy, dpe_device_buffer (when it grows), dpe_viz_render_arrays and
//     dpe_jpeg_blocks_device.  dpe_pm_stage / dpe_pm_stage_resident wait for ev_done only
//     (wait_pending): what they enqueue goes on the context's stream behind its earlier work, and they
//     synchronise it before they return.  dpe_pm_last_stat waits for ev_done and the aux stream.
//   * Entry points that only enqueue STREAM-WAIT with enqueue_stream(): dpe_pm_execute,
//     dpe_pm_export_depth, dpe_state_export_depth, dpe_state_import_depth and
//     dpe_state_render_jpeg_blocks on the caller's stream; dpe_state_save, dpe_state_snapshot and
//     dpe_state_render on the context's.  Those whose work later calls must wait for record ev_done
//     again: dpe_pm_execute, dpe_state_save and dpe_state_snapshot always (mark_pending), the import
//     and the JPEG blocks when they ran on a caller's stream (publish_foreign); the two exports only
//     read, and dpe_state_render synchronises its stream itself.
//   * The EdgeSegment stages and the fusion calls use the context's stream and scratch of their own,
//     and synchronise the stream before they return.  dpe_fusion_tat_image does so too (its kernels
//     have finished when it returns) and then leaves ONE copy in flight: the points of the image, on
//     the aux stream into the caller's buffer, with `tat.ev` recorded behind it.  The next
//     dpe_fusion_tat_image launches its kernels first (they write the other half of the double
//     buffer), then waits for that event before it enqueues its own copy; dpe_fusion_tat_begin,
//     dpe_fusion_tat_wait and dpe_destroy (which synchronises aux) wait for it as well.
// The helpers that carry it (declared and described in dpe_entry.h, for every unit):

hipError_t dpe::wait_pending(DpeContext* c) {
  hipError_t e = hipSuccess;
  if (c->pending) { e = hipEventSynchronize(c->ev_done); c->pending = false; }
  return e;
}

hipError_t dpe::host_wait(DpeContext* c) {
  const hipError_t e = wait_pending(c);
  return e != hipSuccess ? e : hipStreamSynchronize(c->stream);
}

hipError_t dpe::enqueue_stream(DpeContext* c, void* caller_stream, hipStream_t* s) {
  *s = caller_stream ? (hipStream_t)caller_stream : (hipStream_t)c->stream;
  return c->pending ? hipStreamWaitEvent(*s, c->ev_done, 0) : hipSuccess;
}

hipError_t dpe::mark_pending(DpeContext* c, hipStream_t s) {
  const hipError_t e = hipEventRecord(c->ev_done, s);
  if (e == hipSuccess) c->pending = true;
  return e;
}

hipError_t dpe::publish_foreign(DpeContext* c, hipStream_t s) {
  return s == (hipStream_t)c->stream ? hipSuccess : mark_pending(c, s);
}

int dpe::enter(DpeContext* c, bool args_ok, const char* bad_args) {
  g_err.clear();
  if (!c || !args_ok) { g_err = bad_args; return DPE_ERR_ARG; }
  HIPC(hipSetDevice(c->device));
  return DPE_OK;
}

extern "C" {

void dpe_image_cache_clear(DpeContext* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)host_wait(c);
  c->icache.clear();
}

void dpe_destroy(DpeContext* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)host_wait(c);
  (void)hipStreamSynchronize(c->aux);
  delete c;
}

long long dpe_live_device_bytes(void) { return g_live_bytes.load(); }

void dpe_set_timing(DpeContext* c, int enable) { if (c) c->pass.timing = enable != 0; }

}  // extern "C"

// Per-pass constants (restatement of ComputeHomography's plane-independent part, DPE.cu:455-512,
// evaluated in double and rounded once; GenNeighbours' angle constants, DPE.cu:2147-2152).
static void compute_pass_constants(PassConst& pc) {
  const DpeCamera& rc = pc.cams[0];
  const double rK0 = rc.K[0], rK2 = rc.K[2], rK4 = rc.K[4], rK5 = rc.K[5];
  double refC[3];
  for (int j = 0; j < 3; ++j)
    refC[j] = -((double)rc.R[0 + j] * rc.t[0] + (double)rc.R[3 + j] * rc.t[1] + (double)rc.R[6 + j] * rc.t[2]);
  for (int v = 1; v < pc.N; ++v) {
    const DpeCamera& sc = pc.cams[v];
    double srcC[3], Rrel[9], Crel[3], trel[3], T[9];
    for (int j = 0; j < 3; ++j)
      srcC[j] = -((double)sc.R[0 + j] * sc.t[0] + (double)sc.R[3 + j] * sc.t[1] + (double)sc.R[6 + j] * sc.t[2]);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c)
        Rrel[r * 3 + c] = (double)sc.R[r * 3 + 0] * rc.R[c * 3 + 0] + (double)sc.R[r * 3 + 1] * rc.R[c * 3 + 1] +
                          (double)sc.R[r * 3 + 2] * rc.R[c * 3 + 2];
    for (int j = 0; j < 3; ++j) Crel[j] = refC[j] - srcC[j];
    for (int r = 0; r < 3; ++r)
      trel[r] = (double)sc.R[r * 3 + 0] * Crel[0] + (double)sc.R[r * 3 + 1] * Crel[1] + (double)sc.R[r * 3 + 2] * Crel[2];
    for (int r = 0; r < 3; ++r) {
      T[r * 3 + 0] = Rrel[r * 3 + 0] / rK0;
      T[r * 3 + 1] = Rrel[r * 3 + 1] / rK4;
      T[r * 3 + 2] = -Rrel[r * 3 + 0] * rK2 / rK0 - Rrel[r * 3 + 1] * rK5 / rK4 + Rrel[r * 3 + 2];
    }
    const double sK0 = sc.K[0], sK2 = sc.K[2], sK4 = sc.K[4], sK5 = sc.K[5], sK8 = sc.K[8];
    for (int c = 0; c < 3; ++c) {
      pc.vc[v].M[0 + c] = (float)(sK0 * T[0 + c] + sK2 * T[6 + c]);
      pc.vc[v].M[3 + c] = (float)(sK4 * T[3 + c] + sK5 * T[6 + c]);
      pc.vc[v].M[6 + c] = (float)(sK8 * T[6 + c]);
    }
    pc.vc[v].b[0] = (float)(sK0 * trel[0] + sK2 * trel[2]);
    pc.vc[v].b[1] = (float)(sK4 * trel[1] + sK5 * trel[2]);
    pc.vc[v].b[2] = (float)(sK8 * trel[2]);
  }
  pc.kinv0 = (float)(1.0 / rK0);
  pc.kinv4 = (float)(1.0 / rK4);
  pc.kc2 = (float)(rK2 / rK0);
  pc.kc5 = (float)(rK5 / rK4);
  const float angle = 45.0f / pc.P.rotate_time;
  pc.gn_cos = (float)cos((double)angle * M_PI / 180.f);
  pc.gn_sin = (float)sin((double)angle * M_PI / 180.f);
  pc.gn_thr = (float)cos((double)(angle / 2.0f) * M_PI / 180.0f);
  const double sr = tan((double)(angle / 2.0f) * M_PI / 180.0f) * 20;
  const int sri = (sr != sr) ? 0 : (int)sr;
  pc.gn_shift = sri < 1 ? 1 : sri;
  pc.half_rows = std::min(pc.H, 2 * 16 * (((pc.H / 2) + 15) / 16));
  pc.weak_nn = pc.P.weak_radius >= 0 && pc.P.weak_increment > 0 ? (2 * pc.P.weak_radius) / pc.P.weak_increment + 1 : 0;
  pc.tex_wide = tex_wide<TEX_F16>(pc.W);   // the 4-byte layouts' row coefficient fits at every supported width
  static_assert(!tex_wide<TEX_P16>(16000) && !tex_wide<TEX_U8>(16000), "stage_check_args' width limit");
  // float tables of per-pixel expressions that do not depend on the pixel (same bits, pass_tables.h)
  for (int v = 1; v < pc.N; ++v) pc.base_len[v] = baseline_length(rc.c, pc.cams[v].c);
  build_spat36(pc.P.sigma_spatial, pc.spat36);
}

// this unit's own copies of the DPE_DIAG counters (tap_launch.h)
#if DPE_POOL_STATS
DPE_DBG_READER(pool, main, dpe::g_pool, 24)
#endif
#if DPE_LINE_STATS
DPE_DBG_READER(line, main, dpe::g_lstat, 16)
#endif
#if DPE_GN_TIMES
extern "C" void dpe_dbg_gn_times(unsigned int* out, int n) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(dpe::g_gntime), sizeof(unsigned int) * (size_t)(n < (2 << 20) ? n : (2 << 20)));
}
extern "C" void dpe_dbg_gn_counts(unsigned int* out, int n) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(dpe::g_gncnt), sizeof(unsigned int) * (size_t)(n < (6 << 20) ? n : (6 << 20)));
}
#endif
#if DPE_WEAK_STATS
extern "C" void dpe_dbg_weak_stats(unsigned long long out[24], int reset) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(dpe::g_wstat), sizeof(dpe::g_wstat));
  if (reset) { unsigned long long z[24] = {}; (void)hipMemcpyToSymbol(HIP_SYMBOL(dpe::g_wstat), z, sizeof(z)); }
}
#endif

template <class T>
__global__ void k_rescale_nearest(const T* __restrict__ src, int w, int h, T* __restrict__ dst, int nw, int nh, T zero) {
  // RescaleMatToTargetSize (DPE.cpp:1146-1165) with its swapped factors, as host rescale_nearest
  const int c = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y * blockDim.y + threadIdx.y;
  if (c >= nw || r >= nh) return;
  const float scale_x = nw / (float)w, scale_y = nh / (float)h;
  const int o_r = (int)(r / scale_x), o_c = (int)(c / scale_y);
  dst[(size_t)r * nw + c] = (o_r < 0 || o_c < 0 || o_r >= h || o_c >= w) ? zero : src[(size_t)o_r * w + o_c];
}
__global__ void k_rescale_depth(const float4* __restrict__ src, int w, int h, float* __restrict__ dst, int nw, int nh) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y * blockDim.y + threadIdx.y;
  if (c >= nw || r >= nh) return;
  const float scale_x = nw / (float)w, scale_y = nh / (float)h;
  const int o_r = (int)(r / scale_x), o_c = (int)(c / scale_y);
  dst[(size_t)r * nw + c] = (o_r < 0 || o_c < 0 || o_r >= h || o_c >= w) ? 0.0f : src[(size_t)o_r * w + o_c].w;
}

// the pass's initial state in one launch: planes, weak_info and selected views from the staged
// copies, costs and view weights cleared
static_assert(DPE_MAX_IMAGES == 32, "k_pass_init clears 32 view-weight bytes per pixel");
__global__ void __launch_bounds__(256) k_pass_init(const uint4* __restrict__ planes0, const uint8_t* __restrict__ weak0,
                                                   const uint32_t* __restrict__ sel0, uint4* __restrict__ planes,
                                                   uint8_t* __restrict__ weak, uint32_t* __restrict__ sel,
                                                   uint32_t* __restrict__ costs, uint4* __restrict__ vw, size_t L) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L) return;
  planes[i] = planes0[i];
  weak[i] = weak0[i];
  sel[i] = sel0[i];
  costs[i] = 0u;
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  vw[2 * i] = z;
  vw[2 * i + 1] = z;
}

// the state a strong half-sweep reads its neighbours from (planes, costs, selected views before the
// sweep: the red/black same-colour semantics), the three copies in one launch
__global__ void __launch_bounds__(256) k_snapshot(const uint4* __restrict__ planes, const uint32_t* __restrict__ costs,
                                                  const uint32_t* __restrict__ sel, uint4* __restrict__ planes_s,
                                                  uint32_t* __restrict__ costs_s, uint32_t* __restrict__ sel_s, size_t L) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L) return;
  planes_s[i] = planes[i];
  costs_s[i] = costs[i];
  sel_s[i] = sel[i];
}

// where a stage takes the initial state and the source depths from: host buffers (dpe_pm_stage) or
// the resident store (dpe_pm_stage_resident)
struct StageSrc {
  const DpePassState* st = nullptr;   // host initial state
  const ResState* prior = nullptr;    // resident initial state (nullptr: none, FIRST_INIT)
  const ResState* dep[DPE_MAX_IMAGES] = {};   // resident source depths (index 1..N-1)
  bool dep_snap = false;              // read the depths' Jacobi snapshots
};

// ------------------------------------------------------------------------------ staging
// stage_impl's steps, in its order.  Each returns a DPE_* code; all enqueue on the context's stream.

static int stage_check_args(const DpePassInput* in) {   // no HIP call
  if (in->num_images > DPE_MAX_IMAGES) { g_err = "dpe_pm_stage: num_images > 32 (DPE.cpp:762)"; return DPE_ERR_TOO_MANY; }
  if (in->num_images < 2 || in->width <= 0 || in->height <= 0) { g_err = "dpe_pm_stage: bad shape"; return DPE_ERR_ARG; }
  if (in->width > 32000 || in->height > 32000) { g_err = "dpe_pm_stage: image too large for short2 coordinates"; return DPE_ERR_ARG; }
  // tap coordinates on the unit grid of [2^23, 2^24) (pass_common.h kTexMagic): 256 (lim + 1) < 2^22.
  // It also keeps the texel indices below 0xC000 and the 4-byte layouts' row of texels below 64 KiB,
  // which the fast taps' packed texel offset needs (tex_addr.h); the 8-byte layout's rows pass 64 KiB
  // from W = 8190 on, and such a pass runs that layout's kernels with the four-instruction offset
  // (PassConst::tex_wide, set per pass in compute_pass_constants).
  if (in->width > 16000 || in->height > 16000) { g_err = "dpe_pm_stage: image wider or taller than 16000 px"; return DPE_ERR_ARG; }
  const DpePatchMatchParams& P = in->params;
  if (P.rotate_time < 1 || P.rotate_time > 4) { g_err = "dpe_pm_stage: rotate_time must be in [1,4]"; return DPE_ERR_ARG; }
  if (P.strong_increment <= 0 || P.weak_increment <= 0) { g_err = "dpe_pm_stage: increments must be > 0"; return DPE_ERR_ARG; }
  for (int i = 0; i < in->num_images; ++i) if (!in->images[i]) { g_err = "dpe_pm_stage: missing image"; return DPE_ERR_ARG; }
  if ((P.use_edge || P.use_limit) && (!in->edge || !in->edge_low_res || in->low_width <= 0 || in->low_height <= 0)) {
    g_err = "dpe_pm_stage: use_edge/use_limit need edge and edge_low_res"; return DPE_ERR_ARG;
  }
  if (P.use_label && !in->label) { g_err = "dpe_pm_stage: use_label needs label"; return DPE_ERR_ARG; }
  return DPE_OK;
}

static void set_pass_constants(PassConst& pc, const DpePassInput* in) {
  std::memset(&pc, 0, sizeof(pc));
  pc.W = in->width; pc.H = in->height; pc.N = in->num_images;
  pc.P = in->params; pc.P.num_images = pc.N;
  pc.seed32 = (uint32_t)in->seed ^ (uint32_t)(in->seed >> 32);
  pc.salt = in->pass_salt;
  for (int i = 0; i < pc.N; ++i) pc.cams[i] = in->cams[i];
  if (pc.P.use_edge || pc.P.use_limit) { pc.LW = in->low_width; pc.LH = in->low_height; }
  compute_pass_constants(pc);
}

// The half-precision layouts hold every grey level exactly when it is a multiple of 1/4 in
// [0, 255] (IMG_Q: the exact 1/2 and 1/4 INTER_LINEAR downscales of an 8-bit image, the coarse
// pyramid levels of every BASELINE config; the differences b - a of the F16 / P16 texels are then
// exact too); the u8 layout needs integers (IMG_U8: images decoded from 8-bit files).  Identical
// sample values in every layout; the smaller ones gather fewer bytes.
static int image_class(const float* im, size_t L) {
  bool integer = true;
  for (size_t k = 0; k < L; ++k) {
    const float v = im[k];
    if (!(v >= 0.0f && v <= 255.0f)) return IMG_F32;
    const float v4 = v * 4.0f;   // exact (power of two)
    if (v4 != (float)(int)v4) return IMG_F32;
    integer = integer && v == (float)(int)v;
  }
  return integer ? IMG_U8 : IMG_Q;
}

// The texel class of a pass: the narrowest class of its views (IMG_F32 < IMG_Q < IMG_U8), and f32
// when the views' packed arrays would not fit the 32-bit tap offsets.
static int pass_class(int W, int H, int N, const int* view_cls) {
  int cls = (size_t)(W + 2) * (H + 2) * 8 * N < (1ull << 32) ? IMG_U8 : IMG_F32;
  for (int i = 0; i < N; ++i) cls = std::min(cls, view_cls[i]);
  return cls;
}

static size_t quad_plane(int W, int H) { return (size_t)(W + 2) * (H + 2); }   // padded quad texels of one view
static size_t pair_plane(int W, int H) { return (size_t)(W + 3) * (H + 2); }   // TEX_P16 column pairs of one view

// The half-precision layouts of one image: TEX_F16 quads into q16, TEX_P16 column pairs into qp and,
// for an 8-bit image (q8 != nullptr), TEX_U8 quads into q8.
static int build_packed_layouts(hipStream_t s, const float* plain, int W, int H, uint32_t* q8, uint2* q16, uint32_t* qp) {
  const dim3 qb(16, 16), qg((W + 2 + 15) / 16, (H + 2 + 15) / 16), pg((W + 3 + 15) / 16, (H + 2 + 15) / 16);
  k_build_quad8<<<qg, qb, 0, s>>>(plain, q8, q16, W, H);
  k_build_pair16<<<pg, qb, 0, s>>>(plain, qp, W, H);
  HIPC(hipGetLastError());
  return DPE_OK;
}

static int build_f32_quads(hipStream_t s, const float* plain, int W, int H, float4* qf) {
  k_build_quad<<<dim3((W + 2 + 15) / 16, (H + 2 + 15) / 16), dim3(16, 16), 0, s>>>(plain, qf, W, H);
  HIPC(hipGetLastError());
  return DPE_OK;
}

// The packed arrays of a pass of class IMG_U8 / IMG_Q: every view's layout in one allocation (32-bit
// tap offsets), sized for N views and bound into the pass's DevBufs.
static int bind_packed_arrays(DpeContext* c, int cls, int W, int H, int N) {
  const size_t plane = quad_plane(W, H), pplane = pair_plane(W, H);
  DevBufs& B = c->pass.bufs;
  if (cls == IMG_U8) {
    HIPC(c->pass.imgq8_all.ensure(plane * N));
    B.img8 = (const uint8_t*)c->pass.imgq8_all.p; B.img8_view = (uint32_t)(plane * 4);
  }
  HIPC(c->pass.imgq16_all.ensure(plane * N));
  HIPC(c->pass.imgqp_all.ensure(pplane * N));
  B.img16 = (const uint8_t*)c->pass.imgq16_all.p; B.img16_view = (uint32_t)(plane * 8);
  B.imgp = (const uint8_t*)c->pass.imgqp_all.p; B.imgp_view = (uint32_t)(pplane * 4);
  return DPE_OK;
}

// The cache entry of (id, W, H): the one kept, or a new one (upload and the layouts of its own
// class, once).  A new entry first brings the cache under 64 GiB by evicting least recently used
// entries, never one the current call uses (last_use > call_clock).
static int cached_image(DpeContext* c, int id, const float* host, int W, int H, uint64_t call_clock, CachedImage** out) {
  CachedImage* e = nullptr;
  for (auto& q : c->icache)
    if (q->id == id && q->W == W && q->H == H) { e = q.get(); break; }
  if (!e) {
    size_t total = 0;
    for (auto& q : c->icache) total += q->bytes();
    while (total > (64ull << 30)) {
      auto lru = c->icache.end();
      for (auto it = c->icache.begin(); it != c->icache.end(); ++it)
        if ((*it)->last_use <= call_clock && (lru == c->icache.end() || (*it)->last_use < (*lru)->last_use)) lru = it;
      if (lru == c->icache.end()) break;   // only this pass's own views are cached: keep them
      HIPC(hipStreamSynchronize(c->stream));   // nothing enqueued may still read the entry
      total -= (*lru)->bytes();
      c->icache.erase(lru);
    }
    const size_t L = (size_t)W * H;
    auto fresh = std::make_unique<CachedImage>();
    fresh->id = id; fresh->W = W; fresh->H = H;
    fresh->cls = image_class(host, L);
    HIPC(fresh->plain.ensure(L));
    HIPC(hipMemcpyAsync(fresh->plain.p, host, L * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (fresh->cls != IMG_F32) {
      if (fresh->cls == IMG_U8) HIPC(fresh->q8.ensure(quad_plane(W, H)));
      HIPC(fresh->q16.ensure(quad_plane(W, H))); HIPC(fresh->qp.ensure(pair_plane(W, H)));
      TRY(build_packed_layouts(c->stream, fresh->plain.p, W, H, fresh->q8.p, fresh->q16.p, fresh->qp.p));
    }
    e = fresh.get();
    c->icache.push_back(std::move(fresh));   // kept only once it is complete
  }
  e->last_use = ++c->icache_clock;
  *out = e;
  return DPE_OK;
}

// Device-resident images (image_ids): each view from the cache, then the pass's views gathered
// device to device into the packed arrays, or (f32 pass) each entry's f32 quads, built on demand.
static int stage_images_cached(DpeContext* c, const DpePassInput* in) {
  const int W = in->width, H = in->height, N = in->num_images;
  const size_t plane = quad_plane(W, H), pplane = pair_plane(W, H);
  CachedImage* ent[DPE_MAX_IMAGES];
  int view_cls[DPE_MAX_IMAGES];
  const uint64_t call_clock = c->icache_clock;   // entries used by this call have last_use > call_clock
  for (int i = 0; i < N; ++i) {
    TRY(cached_image(c, in->image_ids[i], in->images[i], W, H, call_clock, &ent[i]));
    view_cls[i] = ent[i]->cls;
  }
  const int cls = c->pass.img_cls = pass_class(W, H, N, view_cls);
  DevBufs& B = c->pass.bufs;
  if (cls != IMG_F32) {
    TRY(bind_packed_arrays(c, cls, W, H, N));
    for (int i = 0; i < N; ++i) {
      if (cls == IMG_U8)
        HIPC(hipMemcpyAsync(c->pass.imgq8_all.p + plane * i, ent[i]->q8.p, plane * 4, hipMemcpyDeviceToDevice, c->stream));
      HIPC(hipMemcpyAsync(c->pass.imgq16_all.p + plane * i, ent[i]->q16.p, plane * 8, hipMemcpyDeviceToDevice, c->stream));
      HIPC(hipMemcpyAsync(c->pass.imgqp_all.p + pplane * i, ent[i]->qp.p, pplane * 4, hipMemcpyDeviceToDevice, c->stream));
    }
  } else {
    for (int i = 0; i < N; ++i) {
      if (!ent[i]->qf.p) {
        HIPC(ent[i]->qf.ensure(plane));
        TRY(build_f32_quads(c->stream, ent[i]->plain.p, W, H, ent[i]->qf.p));
      }
      B.imgq[i] = ent[i]->qf.p;
    }
  }
  B.ref = ent[0]->plain.p;
  return DPE_OK;
}

// Images uploaded for this pass only: the layouts of the pass's class built straight into the
// packed arrays, or (f32 pass) into the context's per-view quads.
static int stage_images_direct(DpeContext* c, const DpePassInput* in) {
  const int W = in->width, H = in->height, N = in->num_images;
  const size_t L = (size_t)W * H, plane = quad_plane(W, H), pplane = pair_plane(W, H);
  int view_cls[DPE_MAX_IMAGES];
  for (int i = 0; i < N; ++i)   // one f32 view decides: the rest are not scanned
    view_cls[i] = i > 0 && view_cls[i - 1] == IMG_F32 ? IMG_F32 : image_class(in->images[i], L);
  const int cls = c->pass.img_cls = pass_class(W, H, N, view_cls);
  DevBufs& B = c->pass.bufs;
  if (cls != IMG_F32) TRY(bind_packed_arrays(c, cls, W, H, N));
  for (int i = 0; i < N; ++i) {
    HIPC(c->pass.img_plain[i].ensure(L));
    HIPC(hipMemcpyAsync(c->pass.img_plain[i].p, in->images[i], L * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (cls != IMG_F32) {
      TRY(build_packed_layouts(c->stream, c->pass.img_plain[i].p, W, H, cls == IMG_U8 ? c->pass.imgq8_all.p + plane * i : nullptr,
                               c->pass.imgq16_all.p + plane * i, c->pass.imgqp_all.p + pplane * i));
    } else {
      HIPC(c->pass.imgq[i].ensure(plane));
      TRY(build_f32_quads(c->stream, c->pass.img_plain[i].p, W, H, c->pass.imgq[i].p));
      B.imgq[i] = c->pass.imgq[i].p;
    }
  }
  B.ref = c->pass.img_plain[0].p;
  return DPE_OK;
}

// Source depth maps of the geometric term: from the host, or the resident states (or their Jacobi
// snapshots) rescaled on the device.
static int stage_source_depths(DpeContext* c, const DpePassInput* in, const StageSrc& src) {
  const int W = in->width, H = in->height;
  const size_t L = (size_t)W * H;
  const dim3 rb2(32, 8), rg2((W + 31) / 32, (H + 7) / 8);
  for (int i = 1; i < in->num_images; ++i) {
    HIPC(c->pass.depth[i].ensure(L));
    if (src.st) {
      HIPC(hipMemcpyAsync(c->pass.depth[i].p, in->depths[i], L * sizeof(float), hipMemcpyHostToDevice, c->stream));
    } else {
      const ResState* r = src.dep[i];
      if (src.dep_snap)
        k_rescale_nearest<float><<<rg2, rb2, 0, c->stream>>>(r->snap.p, r->snap_w, r->snap_h, c->pass.depth[i].p, W, H, 0.0f);
      else
        k_rescale_depth<<<rg2, rb2, 0, c->stream>>>(r->planes.p, r->w, r->h, c->pass.depth[i].p, W, H);
      HIPC(hipGetLastError());
    }
    c->pass.bufs.depth[i] = c->pass.depth[i].p;
  }
  return DPE_OK;
}

static int stage_edge_label_maps(DpeContext* c, const DpePassInput* in) {
  const size_t L = (size_t)in->width * in->height, LL = (size_t)in->low_width * in->low_height;
  DevBufs& B = c->pass.bufs;
  if (in->params.use_edge || in->params.use_limit) {
    HIPC(c->pass.edge.ensure(L));
    HIPC(c->pass.edge_low.ensure(LL));
    HIPC(hipMemcpyAsync(c->pass.edge.p, in->edge, L, hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(c->pass.edge_low.p, in->edge_low_res, LL, hipMemcpyHostToDevice, c->stream));
    B.edge = c->pass.edge.p; B.edge_low = c->pass.edge_low.p;
  }
  if (in->params.use_label) {
    HIPC(c->pass.label.ensure(L));
    HIPC(hipMemcpyAsync(c->pass.label.p, in->label, L * sizeof(int), hipMemcpyHostToDevice, c->stream));
    B.label = c->pass.label.p;
  }
  return DPE_OK;
}

// The staged initial state (k_pass_init copies it at the start of every execute): from the host, or
// InuputInitialization's prior (DPE.cpp:845-911) from the resident state, rescaled on the device.
static int stage_initial_state(DpeContext* c, const DpePassInput* in, const StageSrc& src) {
  const DpePatchMatchParams& P = in->params;
  const int W = in->width, H = in->height;
  const size_t L = (size_t)W * H;
  HIPC(c->pass.planes0.ensure(L)); HIPC(c->pass.weak0.ensure(L)); HIPC(c->pass.sel0.ensure(L));
  if (const DpePassState* st = src.st) {
    HIPC(hipMemcpyAsync(c->pass.planes0.p, st->planes, L * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    if (P.use_APD) HIPC(hipMemcpyAsync(c->pass.weak0.p, st->weak_info, L, hipMemcpyHostToDevice, c->stream));
    else HIPC(hipMemsetAsync(c->pass.weak0.p, DPE_STRONG, L, c->stream));   // DPE.cpp:873-881
    HIPC(hipMemcpyAsync(c->pass.sel0.p, st->selected_views, L * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    return DPE_OK;
  }
  const ResState* r = src.prior;
  const dim3 rb2(32, 8), rg2((W + 31) / 32, (H + 7) / 8);
  if (P.state != DPE_FIRST_INIT) {
    k_rescale_nearest<float4><<<rg2, rb2, 0, c->stream>>>(r->planes.p, r->w, r->h, c->pass.planes0.p, W, H, make_float4(0, 0, 0, 0));
    k_rescale_nearest<uint32_t><<<rg2, rb2, 0, c->stream>>>(r->sel.p, r->w, r->h, c->pass.sel0.p, W, H, 0u);
  } else {
    HIPC(hipMemsetAsync(c->pass.planes0.p, 0, L * sizeof(float4), c->stream));
    HIPC(hipMemsetAsync(c->pass.sel0.p, 0, L * sizeof(uint32_t), c->stream));
  }
  if (P.use_APD) k_rescale_nearest<uint8_t><<<rg2, rb2, 0, c->stream>>>(r->weak.p, r->w, r->h, c->pass.weak0.p, W, H, (uint8_t)0);
  else HIPC(hipMemsetAsync(c->pass.weak0.p, DPE_STRONG, L, c->stream));
  HIPC(hipGetLastError());
  return DPE_OK;
}

// The buffers a pass works in, sized for W x H and bound into the pass's DevBufs.
static int ensure_working_set(DpeContext* c, int W, int H) {
  const size_t L = (size_t)W * H;
  HIPC(c->pass.planes.ensure(L)); HIPC(c->pass.planes_snap.ensure(L)); HIPC(c->pass.fit_plane.ensure(L));
  HIPC(c->pass.costs.ensure(L)); HIPC(c->pass.costs_snap.ensure(L)); HIPC(c->pass.complex_.ensure(L));
  HIPC(c->pass.sel.ensure(L)); HIPC(c->pass.sel_snap.ensure(L));
  HIPC(c->pass.weak.ensure(L)); HIPC(c->pass.weak_rel.ensure(L)); HIPC(c->pass.vw.ensure(L * DPE_MAX_IMAGES));
  HIPC(c->pass.nb.ensure(L * 9)); HIPC(c->pass.nearest.ensure(L)); HIPC(c->pass.edge_neigh.ensure(L * 8)); HIPC(c->pass.lab_bound.ensure(L * 8));
  HIPC(c->pass.radius.ensure(L));
  HIPC(c->pass.tab_right.ensure(L)); HIPC(c->pass.tab_down.ensure(L));
  HIPC(c->pass.gn_ovf.ensure(L + 64)); HIPC(c->pass.gn_tab.ensure((size_t)W + H));
  const PassLists lay(W, H, c->pass.hc.half_rows);   // the layout dpe_pm_execute carves them by (pass_lists.h)
  HIPC(c->pass.lists.ensure((size_t)lay.lists_len())); HIPC(c->pass.row_counts.ensure(lay.row_counts_len()));
  HIPC(c->pass.list_totals.ensure(PassLists::kTotals)); HIPC(c->pass.part_cnt.ensure(lay.part_cnt_len()));
  DevBufs& B = c->pass.bufs;
  B.planes = c->pass.planes.p; B.planes_snap = c->pass.planes_snap.p; B.fit_plane = c->pass.fit_plane.p;
  B.planes0 = c->pass.planes0.p;
  B.costs = c->pass.costs.p; B.costs_snap = c->pass.costs_snap.p; B.complex_ = c->pass.complex_.p;
  B.sel = c->pass.sel.p; B.sel_snap = c->pass.sel_snap.p;
  B.weak = c->pass.weak.p; B.weak_rel = c->pass.weak_rel.p; B.vw = c->pass.vw.p;
  B.nb = c->pass.nb.p; B.nearest = c->pass.nearest.p; B.edge_neigh = c->pass.edge_neigh.p; B.lab_bound = c->pass.lab_bound.p;
  B.radius = c->pass.radius.p;
  return DPE_OK;
}

static int stage_impl(DpeContext* c, const DpePassInput* in, const StageSrc& src) {
  Range range_(src.st ? "dpe_pm_stage" : "dpe_pm_stage_resident");
  TRY(stage_check_args(in));
  HIPC(hipSetDevice(c->device));
  HIPC(wait_pending(c));   // an earlier execute on a caller stream may still read what is overwritten here
  set_pass_constants(c->pass.hc, in);
  HIPC(c->pass.dc.ensure(1));
  HIPC(hipMemcpyAsync(c->pass.dc.p, &c->pass.hc, sizeof(PassConst), hipMemcpyHostToDevice, c->stream));
  std::memset(&c->pass.bufs, 0, sizeof(c->pass.bufs));
  TRY(in->image_ids ? stage_images_cached(c, in) : stage_images_direct(c, in));
  if (in->params.geom_consistency) TRY(stage_source_depths(c, in, src));
  TRY(stage_edge_label_maps(c, in));
  TRY(stage_initial_state(c, in, src));
  TRY(ensure_working_set(c, in->width, in->height));
  HIPC(hipStreamSynchronize(c->stream));
  c->pass.staged = true;
#if DPE_GN_ONCE
  c->pass.gn_done_for_stage = false;
#endif
  return DPE_OK;
}

extern "C" int dpe_pm_stage(DpeContext* c, const DpePassInput* in, const DpePassState* st) {
  g_err.clear();
  if (!c || !in || !st || !in->images || !in->cams || !st->planes || !st->weak_info || !st->selected_views) {
    g_err = "dpe_pm_stage: null argument"; return DPE_ERR_ARG;
  }
  if (in->params.geom_consistency) {
    if (!in->depths) { g_err = "dpe_pm_stage: geom_consistency needs depths"; return DPE_ERR_ARG; }
    for (int i = 1; i < in->num_images; ++i) if (!in->depths[i]) { g_err = "dpe_pm_stage: missing source depth"; return DPE_ERR_ARG; }
  }
  StageSrc src;
  src.st = st;
  return stage_impl(c, in, src);
}

extern "C" int dpe_pm_stage_resident(DpeContext* c, const DpePassInput* in, int prior_id) {
  g_err.clear();
  if (!c || !in || !in->images || !in->cams) { g_err = "dpe_pm_stage_resident: null argument"; return DPE_ERR_ARG; }
  const DpePatchMatchParams& P = in->params;
  StageSrc src;
  auto find = [&](int id) -> const ResState* { auto it = c->rstore.find(id); return it == c->rstore.end() ? nullptr : &it->second; };
  if (P.state != DPE_FIRST_INIT || P.use_APD) {
    src.prior = find(prior_id);
    if (!src.prior || !src.prior->full) {
      g_err = "dpe_pm_stage_resident: no resident state of image " + std::to_string(prior_id); return DPE_ERR_STATE;
    }
  }
  if (P.geom_consistency) {
    if (!in->image_ids) { g_err = "dpe_pm_stage_resident: geom_consistency needs image_ids"; return DPE_ERR_ARG; }
    for (int i = 1; i < in->num_images && i < DPE_MAX_IMAGES; ++i) {
      src.dep[i] = find(in->image_ids[i]);
      if (!src.dep[i]) { g_err = "no depth map of source image " + std::to_string(in->image_ids[i]); return DPE_ERR_STATE; }
    }
    src.dep_snap = c->snap_mode;
    if (src.dep_snap)
      for (int i = 1; i < in->num_images && i < DPE_MAX_IMAGES; ++i)
        if (!src.dep[i]->has_snap) { g_err = "no depth snapshot of source image " + std::to_string(in->image_ids[i]); return DPE_ERR_STATE; }
  }
  return stage_impl(c, in, src);
}

// ------------------------------------------------------------------------------ one pass
// dpe_pm_execute: what it records about itself (PassRecorder), its state (PassRun) and its steps, in
// the order of RunPatchMatch's launch sequence (DPE.cu:3150-3226).

static const char* const kClassName[DPE_NUM_CLASSES] = {"setup", "init", "strong", "ransac", "weak", "filter",
                                                         "depth_to_weak", "local_refine"};

// Everything an execute records beside its results: per-class timing events, section counts
// (launches[]), the counting buffer, roctx ranges and the DPE_PHASE_PROF cycle sums.  The launch
// sequence is cut into class sections (setup, init, 5 per iteration, filter, DepthToWeak,
// LocalRefine), each a Section in a scope of its own.
struct PassRecorder {
  DpeContext* c = nullptr;
  hipStream_t s = nullptr;
  const DevBufs* base = nullptr;   // the pass's buffers
  bool timing = false, slot_overflow = false;
  int max_slots = 0, nev = 0;   // timing: (start, end) event pairs available / used
  std::vector<int> ev_class;    //   and the class of each (empty unless timing)

  // Resets the execute's diagnostics on `s_` and marks the start of the pass.  B (which gets the phase
  // buffer of a DPE_PHASE_PROF build) outlives the sections.
  int start(DpeContext* c_, hipStream_t s_, DevBufs& B) {
    c = c_; s = s_; base = &B;
    timing = c->pass.timing;
#if DPE_PHASE_PROF
    HIPC(c->pass.phase.ensure(32 * 64));
    HIPC(hipMemsetAsync(c->pass.phase.p, 0, 32 * 64 * sizeof(unsigned long long), s));
    B.phase = c->pass.phase.p;
#endif
    if (c->pass.counting) {
      HIPC(c->pass.cnt.ensure(DPE_NUM_CLASSES * 4));
      HIPC(hipMemsetAsync(c->pass.cnt.p, 0, DPE_NUM_CLASSES * 4 * sizeof(unsigned long long), s));
    }
    max_slots = 5 + 5 * std::max(0, c->pass.hc.P.max_iterations);
    while (timing && (int)c->ev.size() < 2 * max_slots) {
      Event e;
      HIPC(e.create(hipEventDefault));
      c->ev.push_back(std::move(e));
    }
    ev_class.assign(timing ? max_slots : 0, 0);
    for (int k = 0; k <= DPE_NUM_CLASSES; ++k) c->pass.launches[k] = 0;
    if (timing) (void)hipEventRecord(c->ev_start, s);
    return DPE_OK;
  }

  // One class section: opened where it is declared, closed where its scope ends, also on an early
  // return (the roctx range is popped; the end event is recorded only if the start event was).
  struct Section {
    DevBufs B;   // the pass's buffers, with the class's counters in a counting execute
    PassRecorder& r;
    int slot = -1;
    Section(PassRecorder& r_, int cls) : B(*r_.base), r(r_) {
      roctxRangePushA(kClassName[cls]);
      if (r.c->pass.counting) B.cnt = r.c->pass.cnt.p + 4 * cls;
      r.c->pass.launches[cls]++;
      if (r.timing && r.nev < r.max_slots) { slot = r.nev; r.ev_class[slot] = cls; (void)hipEventRecord(r.c->ev[2 * slot], r.s); }
      else if (r.timing) r.slot_overflow = true;   // more timed sections than slots: finish() fails loudly
    }
    ~Section() {
      if (slot >= 0) { (void)hipEventRecord(r.c->ev[2 * slot + 1], r.s); r.nev++; }
      roctxRangePop();
    }
    Section(const Section&) = delete;
  };

  // After the last launch: timings[] (0: ev_start to the last section's end; 1 + class: the summed
  // sections), the phase report, counts[] (4k + 3: the section counts).
  int finish() {
    if (slot_overflow) {   // per-class times would silently miss launches
      HIPC(hipStreamSynchronize(s));
      g_err = "dpe_pm_execute: more timed launch sections than timing slots (" + std::to_string(max_slots) + ")";
      return DPE_ERR_STATE;
    }
    if (timing && nev > 0) {
      HIPC(hipEventSynchronize(c->ev[2 * nev - 1]));
      for (int k = 0; k <= DPE_NUM_CLASSES; ++k) c->pass.timings[k] = 0.0f;
      float ms = 0;
      (void)hipEventElapsedTime(&ms, c->ev_start, c->ev[2 * nev - 1]);
      c->pass.timings[0] = ms;
      for (int e = 0; e < nev; ++e) {
        (void)hipEventElapsedTime(&ms, c->ev[2 * e], c->ev[2 * e + 1]);
        c->pass.timings[1 + ev_class[e]] += ms;
      }
    }
#if DPE_PHASE_PROF
    unsigned long long ph32[32 * 64], ph[64] = {};
    HIPC(hipMemcpyAsync(ph32, c->pass.phase.p, sizeof(ph32), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    for (int k = 0; k < 32 * 64; ++k) ph[k % 64] += ph32[k];
    unsigned long long tot[4] = {0, 0, 0, 0};
    for (int k = 0; k < 64; ++k) tot[k / 16] += ph[k];
    for (int k = 0; k < 64; ++k)
      if (ph[k]) fprintf(stderr, "PHASE %d.%d %.4e cycles %.1f%%\n", k / 16, k % 16, (double)ph[k], 100.0 * ph[k] / tot[k / 16]);
#endif
    if (c->pass.counting) {
      HIPC(hipMemcpyAsync(c->pass.counts, c->pass.cnt.p, sizeof(c->pass.counts), hipMemcpyDeviceToHost, s));
      HIPC(hipStreamSynchronize(s));
      for (int k = 0; k < DPE_NUM_CLASSES; ++k) c->pass.counts[4 * k + 3] = (unsigned long long)c->pass.launches[k];
    }
    return DPE_OK;
  }
};
using Section = PassRecorder::Section;

// The state of one execute.  Every pointer into the list buffers comes from `lay` (pass_lists.h).
// Streams: overlapped schedule, `s` is the pass stream and `a` the context's aux stream; one-stream
// schedule (timed and counting executes, whose per-class events must not overlap; DPE_OVERLAP=0, for
// profiles whose kernel durations must not; a pass without iterations, since the join into `s` sits
// in the first strong half-sweep): a == s, and fork() and the joins do nothing.
struct PassRun {
  DpeContext* c;
  hipStream_t s, a;
  bool overlap;
  const PassConst& pc;   // host copy of the pass constants
  const PassConst* dpc;  //   and the device copy the kernels read
  DevBufs B;
  PassLists lay;
  size_t L;              // pixels
  int nv;                // source views
  bool gn_skip = false;  // DPE_GN_ONCE builds: GenNeighbours' outputs of this staged state are kept
  PassRecorder rec;

  PassRun(DpeContext* c_, hipStream_t s_)
      : c(c_), s(s_), a(s_), pc(c_->pass.hc), dpc(c_->pass.dc.p), B(c_->pass.bufs), lay(pc.W, pc.H, pc.half_rows),
        L((size_t)pc.W * pc.H), nv(pc.N - 1) {
    static const bool overlap_env = [] { const char* e = getenv("DPE_OVERLAP"); return !(e && atoi(e) == 0); }();   // once per process
    overlap = overlap_env && !c->pass.timing && !c->pass.counting && pc.P.max_iterations >= 1;
    if (overlap) a = c->aux;
    B.cnt = nullptr;
    const char* e = getenv("DPE_XCD_ROWS");   // tuning knob, read on every execute: block rows per XCD
    B.xcd_rows = e ? atoi(e) : kDefaultXcdRows;   //   chunk (see xcd_remap); 0 disables
  }
  // `a` continues from here on `s`
  hipError_t fork(hipEvent_t ev) const {
    const hipError_t e = overlap ? hipEventRecord(ev, s) : hipSuccess;
    return e != hipSuccess || !overlap ? e : hipStreamWaitEvent(a, ev, 0);
  }
  // `s` continues after what `a` holds now: join(), or its two halves around launches on `s`
  hipError_t aux_done(hipEvent_t ev) const { return overlap ? hipEventRecord(ev, a) : hipSuccess; }
  hipError_t wait_aux(hipEvent_t ev) const { return overlap ? hipStreamWaitEvent(s, ev, 0) : hipSuccess; }
  hipError_t join(hipEvent_t ev) const { const hipError_t e = aux_done(ev); return e != hipSuccess ? e : wait_aux(ev); }

  int* list(PassLists::Region r) const { return c->pass.lists.p + r.off; }
  int* rows(PassLists::Region r) const { return c->pass.row_counts.p + r.off; }
  int* total(int slot) const { return c->pass.list_totals.p + slot; }
  int* chunk_counts(int colour) const { return c->pass.part_cnt.p + lay.chunk_counts(colour).off; }
  dim3 px_grid() const { return dim3((pc.W + 15) / 16, (pc.H + 15) / 16); }   // of kPxBlock threads: one per pixel
};
static const dim3 kPxBlock(16, 16);

// One pixel-list build (pass_sweep.h, MODE 0 / 1 / 2) on stream `st`: row counts, their scan, fill.
// MODE 0 builds the four sweep lists, consecutive from `list` with their totals consecutive from
// `total`; `stride` lies between them (the one-list modes never use theirs).
template <int MODE>
static void build_lists(const PassRun& X, hipStream_t st, const DevBufs& Bl, PassLists::Region rows, int total,
                        PassLists::Region list) {
  const unsigned grid = (unsigned)(((MODE == 1 ? X.pc.H : X.pc.half_rows) + 3) / 4);   // a wave per row (list_rows<MODE>)
  const long stride = MODE == 1 ? X.lay.px() : list.len;
  int* rc = X.rows(rows);
  k_list_count<MODE><<<grid, 256, 0, st>>>(X.dpc, Bl, rc);
  k_list_scan<MODE><<<1, 64 * list_count<MODE>(), 0, st>>>(X.dpc, rc, X.total(total));
  k_list_fill<MODE><<<grid, 256, 0, st>>>(X.dpc, Bl, rc, X.list(list), stride);
}
// the per-colour strong / weak lists of the sweeps, on `s`
static void sweep_lists(const PassRun& X, const DevBufs& Bl) {
  build_lists<0>(X, X.s, Bl, X.lay.sweep_rows(), PassLists::total_sweep(0, 0), X.lay.sweep(0, 0));
}

// The part of the initial state that the setup chain reads first (or, after it joins the pass
// stream, RANSACToGetFitPlane and the weak sweeps): cleared on the setup chain's stream `st`.
static int clear_setup_state(const PassRun& X, hipStream_t st) {
  const DevBufs& B = X.B;
  const size_t L = X.L;
  HIPC(hipMemsetAsync(B.fit_plane, 0, L * sizeof(float4), st));
  HIPC(hipMemsetAsync(B.complex_, 0, L * sizeof(float), st));
  if (!X.gn_skip) HIPC(hipMemsetAsync(B.weak_rel, 0xFF, L, st));   // GenNeighbours writes 0 / 1 for every WEAK pixel
  if (!X.gn_skip) HIPC(hipMemsetAsync(B.nb, 0xFF, L * 9 * sizeof(short2), st));
  HIPC(hipMemsetAsync(B.nearest, 0xFF, L * sizeof(short2), st));
  HIPC(hipMemsetAsync(B.edge_neigh, 0xFF, L * 8 * sizeof(short2), st));
  HIPC(hipMemsetAsync(B.lab_bound, 0xFF, L * 8 * sizeof(short2), st));
  HIPC(hipMemsetAsync(B.radius, 0, L * sizeof(int), st));
  return DPE_OK;
}

// GenNeighbours, one thread per pixel of the all-WEAK list, on `a`.
static int gen_neighbours(PassRun& X, const DevBufs& Bc) {
  DpeContext* c = X.c;
  const hipStream_t a = X.a;
  const int* weak_list = X.list(X.lay.all_weak());
  const int* cnt = X.total(PassLists::kTotAllWeak);
  if (!X.gn_skip) {
    // rotate_time is in [1,4] (stage_check_args): both kernels' point stores rely on it.
    // The scratch-free kernel; pixels with more support points than its LDS slots (none at the
    // BASELINE workloads) or a NaN go to the scratch kernel, a small persistent grid that loops over
    // that overflow list (its count: the GenNeighbours-overflow total, dpe_pm_last_stat)
    int* ovf = X.total(PassLists::kTotGnOverflow);
    k_gn_tables<<<(unsigned)((X.pc.W + X.pc.H + 255) / 256), 256, 0, a>>>(X.dpc, c->pass.gn_tab.p);
    HIPC(hipMemsetAsync(ovf, 0, sizeof(int), a));
    const unsigned gg = (unsigned)((X.L + kGnBT - 1) / kGnBT);
    if (c->pass.gn_slots == 8)   // test setting: most pixels overflow into the scratch kernel
      k_gen_neighbours_lds<8><<<gg, kGnBT, 0, a>>>(X.dpc, Bc, weak_list, cnt, c->pass.gn_tab.p, c->pass.gn_ovf.p, ovf);
    // at most 16 x rotate_time support points; 32 slots asked for above rotate_time 2 is a test setting
    // too: the pixels with more than 32 points overflow
    else if (c->pass.gn_slots == 32 || (X.pc.P.rotate_time <= 2 && c->pass.gn_slots != 64))
      k_gen_neighbours_lds<32><<<gg, kGnBT, 0, a>>>(X.dpc, Bc, weak_list, cnt, c->pass.gn_tab.p, c->pass.gn_ovf.p, ovf);
    else
      k_gen_neighbours_lds<64><<<gg, kGnBT, 0, a>>>(X.dpc, Bc, weak_list, cnt, c->pass.gn_tab.p, c->pass.gn_ovf.p, ovf);
    k_gen_neighbours<<<kGnOvfBlocks, 256, 0, a>>>(X.dpc, Bc, c->pass.gn_ovf.p, ovf);
  }
#if DPE_GN_ONCE
  if (!X.gn_skip) {   // kept for the next executes of this staged state (see dpe_pm_execute)
    HIPC(c->pass.gn_complex.ensure(X.L));
    HIPC(hipMemcpyAsync(c->pass.gn_complex.p, X.B.complex_, X.L * sizeof(float), hipMemcpyDeviceToDevice, a));
    c->pass.gn_done_for_stage = true;
  }
#endif
  return DPE_OK;
}

// The setup chain: GenEdgeInform and its edge rays, FindNearestStrongPoint's tables, the all-WEAK
// list, GenNeighbours, NeigbourUpdate, then the pixel lists.  Streams: all of it on `a`; overlapped,
// `s` first builds the pre-GenNeighbours sweep lists and forks `a`, which marks ev_ei behind the
// edge rays and ev_join at its end.
// Why the fork is legal: GenNeighbours + NeigbourUpdate only decide which WEAK pixels join the strong
// lists.  Nothing RandomInitialization or the first strong half-sweep (iteration 0, colour 0) reads
// is written by them, and GenNeighbours reads the staged planes, not the ones those two rewrite; that
// half-sweep needs GenEdgeInform's edge rays only (ev_ei).  So it runs over the pre-GenNeighbours
// colour-0 strong list, and the colour-0 pixels whose GenNeighbours failed (NeigbourUpdate makes them
// UNKNOWN; the failed list) get the same half-sweep, same snapshot, once the streams join
// (strong_half_sweep).  Pixels of one half-sweep are independent, so this is the reference's order of
// results (GPU test test_overlapped_and_sequential_schedules_agree).
static int setup_chain(PassRun& X) {
  DpeContext* c = X.c;
  const PassConst& pc = X.pc;
  const hipStream_t a = X.a;
  Section sec(X.rec, DPE_CLASS_SETUP);
  const DevBufs& Bc = sec.B;
  if (X.overlap) sweep_lists(X, Bc);   // pre-GenNeighbours: the colour-0 strong list is the one used
  HIPC(X.fork(c->ev_fork));
  TRY(clear_setup_state(X, a));
  k_gen_edge_inform<<<X.px_grid(), kPxBlock, 0, a>>>(X.dpc, Bc);
  if (pc.P.use_edge) k_edge_rays<<<(unsigned)(3 * (pc.W + pc.H) - 2), 64, 0, a>>>(X.dpc, Bc);
#if DPE_GN_ONCE   // GenEdgeInform rewrites complex_: GenNeighbours' kept one is restored after it
  if (X.gn_skip) HIPC(hipMemcpyAsync(X.B.complex_, c->pass.gn_complex.p, X.L * sizeof(float), hipMemcpyDeviceToDevice, a));
#endif
  HIPC(X.aux_done(c->ev_ei));
  k_strong_tables_scan<<<(unsigned)(pc.W + pc.H), 64, 0, a>>>(X.dpc, Bc, c->pass.tab_right.p, c->pass.tab_down.p);
  k_find_nearest_strong<<<X.px_grid(), kPxBlock, 0, a>>>(X.dpc, Bc, c->pass.tab_right.p, c->pass.tab_down.p);
  build_lists<1>(X, a, Bc, X.lay.all_weak_rows(), PassLists::kTotAllWeak, X.lay.all_weak());
  TRY(gen_neighbours(X, Bc));
  k_neighbour_update<<<X.px_grid(), kPxBlock, 0, a>>>(X.dpc, Bc);
  // weak_info is fixed from here until DepthToWeak.  Overlapped, `s` may be inside its first strong
  // half-sweep: `a` builds the failed list only (regions of its own in every list buffer), and `s`
  // rebuilds the sweep lists after the join
  if (X.overlap) build_lists<2>(X, a, Bc, X.lay.failed_rows(), PassLists::kTotFailed, X.lay.failed());
  else sweep_lists(X, Bc);
  HIPC(X.aux_done(c->ev_join));
  return DPE_OK;
}

// RandomInitialization, on `s`; the strong sweeps behind it read GenEdgeInform's rays (ev_ei).
static int random_initialization(PassRun& X) {
  {
    Section sec(X.rec, DPE_CLASS_INIT);
    if (X.c->pass.img_cls != IMG_F32) k_random_init<kTexInit><<<X.px_grid(), kPxBlock, 0, X.s>>>(X.dpc, sec.B);
    else k_random_init<TEX_F32><<<X.px_grid(), kPxBlock, 0, X.s>>>(X.dpc, sec.B);
  }
  HIPC(X.wait_aux(X.c->ev_ei));
  HIPC(hipGetLastError());
  return DPE_OK;
}

// CheckerboardPropagationStrong + refinement over one list, on `s`
static void strong_sweep(const PassRun& X, const DevBufs& Bs, int it, PassLists::Region list, int total) {
  const bool edge = X.pc.P.use_edge;
  const int P = edge ? 4 : 8, C = edge ? 16 : 8;
  const size_t lds = (size_t)kBwStrong * strong_lds_per_wave(P, C, X.nv) * sizeof(float);
  const unsigned grid = (unsigned)((X.L / 2 + 1 + kBwStrong * P - 1) / (kBwStrong * P));
  launch_strong(edge, X.c->pass.img_cls, grid, lds, X.s, X.dpc, Bs, it, X.list(list), X.total(total));
}

// One colour's strong half-sweep over the snapshot of the state before it, on `s`.  Overlapped, the
// first one of the pass (over the pre-GenNeighbours list) is where `s` joins the setup chain
// (ev_join): it then sweeps the failed list over the same snapshot and builds the final sweep lists.
static int strong_half_sweep(PassRun& X, int it, int colour) {
  const DevBufs& B = X.B;
  k_snapshot<<<(unsigned)((X.L + 255) / 256), 256, 0, X.s>>>((const uint4*)B.planes, (const uint32_t*)B.costs, B.sel,
                                                               (uint4*)B.planes_snap, (uint32_t*)B.costs_snap, B.sel_snap, X.L);
  Section sec(X.rec, DPE_CLASS_STRONG);
  strong_sweep(X, sec.B, it, X.lay.sweep(colour, 0), PassLists::total_sweep(colour, 0));
  if (X.overlap && it == 0 && colour == 0) {
    HIPC(X.wait_aux(X.c->ev_join));
    strong_sweep(X, sec.B, it, X.lay.failed(), PassLists::kTotFailed);
    sweep_lists(X, sec.B);
  }
  return DPE_OK;
}

// CheckerboardPropagationWeak + refinement over one colour's weak list, on stream `st`
static void weak_sweep(const PassRun& X, const DevBufs& Bc, int it, int colour, hipStream_t st) {
  const int* lst = X.list(X.lay.sweep(colour, 1));
  const int* cnt = X.total(PassLists::total_sweep(colour, 1));
  if (X.pc.P.use_radius) {   // the fits just set the radii: partition the list by centre-patch side
    const unsigned pg = (unsigned)X.lay.chunks();
    int* pcnt = X.chunk_counts(colour);
    int* tot = X.total(PassLists::total_side(colour));
    int* out = X.list(X.lay.side(colour));
    k_part_count<<<pg, 256, 0, st>>>(X.dpc, Bc, lst, cnt, pcnt);
    k_part_scan<<<1, 256, 0, st>>>(cnt, pcnt, tot);
    k_part_fill<<<pg, 256, 0, st>>>(X.dpc, Bc, lst, cnt, pcnt, tot, out);
    lst = out;
  }
  constexpr int C = kWeakLanes, P = 64 / C;
  const size_t per_wave = (size_t)P * weak_lds_per_pixel(X.nv) * sizeof(float);
  const int wpb = per_wave * 4 <= 64 * 1024 ? 4 : (per_wave * 2 <= 64 * 1024 ? 2 : 1);
  const unsigned grid = (unsigned)((X.L / 2 + 1 + wpb * P - 1) / (wpb * P));
  // U8 texels for 8-bit images; F16 (exact for quarter-integer grey levels) for the coarse levels
  if (X.c->pass.img_cls == IMG_U8) k_weak_coop<kTexWeak, C><<<grid, 64 * wpb, per_wave * wpb, st>>>(X.dpc, Bc, it, lst, cnt);
  else if (X.c->pass.img_cls == IMG_Q && X.pc.tex_wide) k_weak_coop<TEX_F16W, C><<<grid, 64 * wpb, per_wave * wpb, st>>>(X.dpc, Bc, it, lst, cnt);
  else if (X.c->pass.img_cls == IMG_Q) k_weak_coop<TEX_F16, C><<<grid, 64 * wpb, per_wave * wpb, st>>>(X.dpc, Bc, it, lst, cnt);
  else k_weak_coop<TEX_F32, C><<<grid, 64 * wpb, per_wave * wpb, st>>>(X.dpc, Bc, it, lst, cnt);
}

// RANSACToGetFitPlane and the weak sweeps of one iteration.  Streams: colour 0 on `s`, colour 1 on
// `a`, forked before the fits (the colour-1 fit must not wait for the colour-0 one) and joined behind
// the sweeps.
// Why the fork is legal: a weak sweep reads only STRONG pixels' state besides its own pixel (planes
// and selected views of the GenNeighbours support points, DPE.cu:1690-1725; the NCC-New patches come
// from the images) and writes only its own pixel, so the two colours are independent (their launch
// tails overlap).  A fit reads STRONG pixels and writes its own pixel's fit plane, which only its
// own weak update reads, so each colour's fits run on that colour's stream just before its sweep.
static int fits_and_weak_sweeps(PassRun& X, int it) {
  const unsigned rl_grid = (unsigned)((X.L / 2 + 1 + kRansacThreads - 1) / kRansacThreads);
  HIPC(X.fork(X.c->ev_fork));
  {
    Section sec(X.rec, DPE_CLASS_RANSAC);
    for (int colour = 1; colour >= 0; --colour)
      k_ransac_fit<<<rl_grid, kRansacThreads, 0, colour == 1 ? X.a : X.s>>>(
          X.dpc, sec.B, it, X.list(X.lay.sweep(colour, 1)), X.total(PassLists::total_sweep(colour, 1)));
  }
  for (int colour = 0; colour < 2; ++colour) {
    Section sec(X.rec, DPE_CLASS_WEAK);
    weak_sweep(X, sec.B, it, colour, colour == 1 ? X.a : X.s);
  }
  HIPC(X.join(X.c->ev_join));
  HIPC(hipGetLastError());
  return DPE_OK;
}

// GetDepthandNormal and CheckerboardFilterStrong, on `s`
static void filter(PassRun& X) {
  const dim3 hb(32, 4), hg((((X.pc.W + 1) / 2) + 31) / 32, (X.pc.half_rows + 3) / 4);   // hb: 32 x 4 = kFilterThreads
  Section sec(X.rec, DPE_CLASS_FILTER);
  k_depth_normal<<<X.px_grid(), kPxBlock, 0, X.s>>>(X.dpc, sec.B);
  for (int colour = 0; colour < 2; ++colour) k_filter<<<hg, hb, 0, X.s>>>(X.dpc, sec.B, colour);
}

// DepthToWeak (LocalRefine fused for interior pixels) on `s`, and LocalRefine on the 6-px border that
// DepthToWeak leaves to it: overlapped on `a` beside DepthToWeak, else on `s` behind it.
// Why the fork is legal: the border LocalRefine reads and writes only its own pixel's plane besides
// the images and source depths (DPE.cu:2749-2835), and DepthToWeak writes only interior pixels.  The
// border kernel is launched first: it is small and would otherwise wait for DepthToWeak's slots.
static int depth_to_weak(PassRun& X) {
  DpeContext* c = X.c;
  auto border_local_refine = [&](hipStream_t st) {
    Section sec(X.rec, DPE_CLASS_LOCAL_REFINE);
    launch_local_refine(c->pass.img_cls, X.pc.tex_wide, (long)X.L, X.pc.W, X.pc.H, X.nv, st, X.dpc, sec.B);
  };
  HIPC(X.fork(c->ev_fork));
  if (X.overlap) border_local_refine(X.a);
  HIPC(X.aux_done(c->ev_join));
  {
    Section sec(X.rec, DPE_CLASS_DEPTH_TO_WEAK);
    launch_depth_to_weak(c->pass.img_cls, X.pc.tex_wide, (long)X.L, X.s, X.dpc, sec.B);
  }
  HIPC(X.wait_aux(c->ev_join));
  if (!X.overlap) border_local_refine(X.s);
  HIPC(hipGetLastError());
  return DPE_OK;
}

#if DPE_GN_ONCE
// Timing builds only (pass_common.h): GenNeighbours runs in the first execute after a stage and its
// outputs (nb, weak_rel, and complex_, which GenEdgeInform rewrites: restored after it) are kept for
// the next executes of the same staged state, which then skip it -- the same results (GenNeighbours
// depends only on the staged state), and the pass time without GenNeighbours on the critical path.
// An execute that fails forgets them.
struct GnGuard {
  DpeContext* c;
  bool ok = false;
  ~GnGuard() { if (!ok) c->pass.gn_done_for_stage = false; }
};
#endif

extern "C" int dpe_pm_execute(DpeContext* c, void* stream_) {
  TRY(enter(c, true, "dpe_pm_execute: null context"));
  if (!c->pass.staged) { g_err = "dpe_pm_execute: call dpe_pm_stage first"; return DPE_ERR_STATE; }
  Range range_("dpe_pm_execute");
  hipStream_t s;
  // a previous execute, possibly on another stream, still uses the working buffers this one resets
  HIPC(enqueue_stream(c, stream_, &s));
  PassRun X(c, s);
  TRY(X.rec.start(c, s, X.B));
#if DPE_GN_ONCE
  X.gn_skip = c->pass.gn_done_for_stage;
  GnGuard gn_guard{c};
#endif
  // initial state (the reference uploads it in CudaSpaceInitialization, DPE.cpp:964-1015); the rest
  // of it is cleared by the setup chain
  k_pass_init<<<(unsigned)((X.L + 255) / 256), 256, 0, s>>>((const uint4*)c->pass.planes0.p, c->pass.weak0.p, c->pass.sel0.p, (uint4*)X.B.planes,
                                                            X.B.weak, X.B.sel, (uint32_t*)X.B.costs, (uint4*)X.B.vw, X.L);
  TRY(setup_chain(X));
  TRY(random_initialization(X));
  for (int it = 0; it < X.pc.P.max_iterations; ++it) {
    for (int colour = 0; colour < 2; ++colour) TRY(strong_half_sweep(X, it, colour));
    HIPC(hipGetLastError());
    TRY(fits_and_weak_sweeps(X, it));
  }
  filter(X);
  TRY(depth_to_weak(X));
  TRY(X.rec.finish());
  HIPC(mark_pending(c, s));
#if DPE_GN_ONCE
  gn_guard.ok = true;
#endif
  return DPE_OK;
}

extern "C" int dpe_pm_fetch(DpeContext* c, const DpePassState* st) {
  TRY(enter(c, st != nullptr, "dpe_pm_fetch: null argument"));
  if (!c->pass.staged) { g_err = "dpe_pm_fetch: nothing staged"; return DPE_ERR_STATE; }
  Range range_("dpe_pm_fetch");
  const size_t L = (size_t)c->pass.hc.W * c->pass.hc.H;
  HIPC(host_wait(c));
  if (st->planes) HIPC(hipMemcpy(st->planes, c->pass.bufs.planes, L * sizeof(float4), hipMemcpyDeviceToHost));
  if (st->weak_info) HIPC(hipMemcpy(st->weak_info, c->pass.bufs.weak, L, hipMemcpyDeviceToHost));
  if (st->selected_views) HIPC(hipMemcpy(st->selected_views, c->pass.bufs.sel, L * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (st->costs) HIPC(hipMemcpy(st->costs, c->pass.bufs.costs, L * sizeof(float), hipMemcpyDeviceToHost));
  return DPE_OK;
}

extern "C" int dpe_pm_run(DpeContext* c, const DpePassInput* in, const DpePassState* st) {
  int r = dpe_pm_stage(c, in, st);
  if (r) return r;
  r = dpe_pm_execute(c, nullptr);
  if (r) return r;
  return dpe_pm_fetch(c, st);
}

extern "C" int dpe_pm_last_timings(DpeContext* c, float* out, int n) {
  if (!c || !out) return 0;
  const int m = n < DPE_NUM_CLASSES + 1 ? n : DPE_NUM_CLASSES + 1;
  for (int i = 0; i < m; ++i) out[i] = c->pass.timings[i];
  return m;
}

extern "C" void dpe_set_counting(DpeContext* c, int enable) { if (c) c->pass.counting = enable != 0; }

extern "C" int dpe_set_option(DpeContext* c, int option, int value) {
  g_err.clear();   // (touches no device)
  if (!c) { g_err = "dpe_set_option: null context"; return DPE_ERR_ARG; }
  if (option == DPE_OPT_GN_SLOTS && (value == 0 || value == 8 || value == 32 || value == 64)) { c->pass.gn_slots = value; return DPE_OK; }
  g_err = "dpe_set_option: unknown option or value";
  return DPE_ERR_ARG;
}

extern "C" long long dpe_pm_last_stat(DpeContext* c, int stat) {
  if (c && c->pass.staged && stat == DPE_STAT_TEX_CLASS) return c->pass.img_cls;
  if (!c || !c->pass.staged || stat != DPE_STAT_GN_DEFERRED || !c->pass.list_totals.p) return -1;
  int v = 0;   // waits for this context's pass only (not the whole device)
  if (hipSetDevice(c->device) != hipSuccess || wait_pending(c) != hipSuccess || hipStreamSynchronize(c->aux) != hipSuccess ||
      hipMemcpyAsync(&v, c->pass.list_totals.p + PassLists::kTotGnOverflow, sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess)
    return -1;
  return v;
}

extern "C" int dpe_pm_last_counts(DpeContext* c, unsigned long long* out, int n) {
  if (!c || !out) return 0;
  const int m = n < DPE_NUM_CLASSES * 4 ? n : DPE_NUM_CLASSES * 4;
  for (int i = 0; i < m; ++i) out[i] = c->pass.counts[i];
  return m;
}
