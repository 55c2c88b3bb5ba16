// dpe_mvs.hip — the C-ABI library (include/dpe_mvs.h): context, HBM staging and the launch
// sequence of one PatchMatch pass on gfx950.
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
#include <rocprofiler-sdk-roctx/roctx.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "pass_tables.h"
#include "pass_kernels.h"
#include "pass_refine.h"
#include "pass_fusion.h"
#include "pass_fusion_tat.h"
#include "pass_sweep.h"
#include "pass_edges.h"
#include "pass_viz.h"
#include "tap_launch.h"
#include "dpe_context.h"

using namespace dpe;

static const int kDefaultXcdRows = 1;
static constexpr int kWeakLanes = 16;   // lanes per weak pixel in k_weak_coop

namespace {

thread_local std::string g_err;

// roctx ranges (SURVEY.md §5 tracing): host-side enqueue regions of the pass, visible in
// `rocprofv3 --marker-trace` beside the kernel trace
struct Range {
  explicit Range(const char* m) { roctxRangePushA(m); }
  ~Range() { roctxRangePop(); }
  Range(const Range&) = delete;
  Range& operator=(const Range&) = delete;
};

#define HIPC(expr)                                                                  \
  do {                                                                              \
    hipError_t e_ = (expr);                                                         \
    if (e_ != hipSuccess) {                                                         \
      g_err = std::string(#expr) + ": " + hipGetErrorString(e_);                    \
      return DPE_ERR_HIP;                                                           \
    }                                                                               \
  } while (0)

// a step of a longer sequence: its DPE_* code ends the caller unless it is DPE_OK
#define TRY(expr)                                                                   \
  do {                                                                              \
    if (const int rc_ = (expr); rc_ != DPE_OK) return rc_;                          \
  } while (0)

}  // namespace

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
      c->ev_ei.create() != hipSuccess || c->ev_done.create() != hipSuccess || c->ev_tat.create() != hipSuccess ||
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
//     the aux stream into the caller's buffer, with `ev_tat` recorded behind it.  The next
//     dpe_fusion_tat_image launches its kernels first (they write the other half of the double
//     buffer), then waits for that event before it enqueues its own copy; dpe_fusion_tat_begin,
//     dpe_fusion_tat_wait and dpe_destroy (which synchronises aux) wait for it as well.

// Host-waits for the work of the last dpe_pm_execute, which may have been enqueued on a caller
// stream: staging, fetching and freeing must not overwrite or release buffers that pass still uses.
static hipError_t wait_pending(DpeContext* c) {
  hipError_t e = hipSuccess;
  if (c->pending) { e = hipEventSynchronize(c->ev_done); c->pending = false; }
  return e;
}

// Host-waits until the context is quiet: the pending work, then everything on its own stream.
static hipError_t host_wait(DpeContext* c) {
  const hipError_t e = wait_pending(c);
  return e != hipSuccess ? e : hipStreamSynchronize(c->stream);
}

// The stream an entry point enqueues on (the caller's, or the context's for nullptr), after making it
// wait for the pending work.
static hipError_t enqueue_stream(DpeContext* c, void* caller_stream, hipStream_t* s) {
  *s = caller_stream ? (hipStream_t)caller_stream : (hipStream_t)c->stream;
  return c->pending ? hipStreamWaitEvent(*s, c->ev_done, 0) : hipSuccess;
}

// Makes the work enqueued on `s` so far the pending work that later calls wait for.
static hipError_t mark_pending(DpeContext* c, hipStream_t s) {
  const hipError_t e = hipEventRecord(c->ev_done, s);
  if (e == hipSuccess) c->pending = true;
  return e;
}

// The same for work that went on a caller's stream; the context's own stream orders its work itself.
static hipError_t publish_foreign(DpeContext* c, hipStream_t s) {
  return s == (hipStream_t)c->stream ? hipSuccess : mark_pending(c, s);
}

// The prologue of an entry point: clears the thread's error, refuses a null context or bad arguments
// with DPE_ERR_ARG and `bad_args`, and selects the context's device.
static int enter(DpeContext* c, bool args_ok, const char* bad_args) {
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

void dpe_set_timing(DpeContext* c, int enable) { if (c) c->timing = enable != 0; }

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
  // float tables of per-pixel expressions that do not depend on the pixel (same bits, pass_tables.h)
  for (int v = 1; v < pc.N; ++v) pc.base_len[v] = baseline_length(rc.c, pc.cams[v].c);
  build_spat36(pc.P.sigma_spatial, pc.spat36);
}

#if DPE_POOL_STATS
extern "C" void dpe_dbg_pool_stats_main(unsigned long long out[24], int reset) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(dpe::g_pool), sizeof(dpe::g_pool));
  if (reset) { unsigned long long z[24] = {}; (void)hipMemcpyToSymbol(HIP_SYMBOL(dpe::g_pool), z, sizeof(z)); }
}
#endif
#if DPE_LINE_STATS
extern "C" void dpe_dbg_line_stats_main(unsigned long long out[16], int reset) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(dpe::g_lstat), sizeof(dpe::g_lstat));
  if (reset) { unsigned long long z[16] = {}; (void)hipMemcpyToSymbol(HIP_SYMBOL(dpe::g_lstat), z, sizeof(z)); }
}
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
  // tap coordinates on the unit grid of [2^23, 2^24) (pass_common.h kTexMagic): 256 (lim + 1) < 2^22
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
  DevBufs& B = c->bufs;
  if (cls == IMG_U8) {
    HIPC(c->imgq8_all.ensure(plane * N));
    B.img8 = (const uint8_t*)c->imgq8_all.p; B.img8_view = (uint32_t)(plane * 4);
  }
  HIPC(c->imgq16_all.ensure(plane * N));
  HIPC(c->imgqp_all.ensure(pplane * N));
  B.img16 = (const uint8_t*)c->imgq16_all.p; B.img16_view = (uint32_t)(plane * 8);
  B.imgp = (const uint8_t*)c->imgqp_all.p; B.imgp_view = (uint32_t)(pplane * 4);
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
  const int cls = c->img_cls = pass_class(W, H, N, view_cls);
  DevBufs& B = c->bufs;
  if (cls != IMG_F32) {
    TRY(bind_packed_arrays(c, cls, W, H, N));
    for (int i = 0; i < N; ++i) {
      if (cls == IMG_U8)
        HIPC(hipMemcpyAsync(c->imgq8_all.p + plane * i, ent[i]->q8.p, plane * 4, hipMemcpyDeviceToDevice, c->stream));
      HIPC(hipMemcpyAsync(c->imgq16_all.p + plane * i, ent[i]->q16.p, plane * 8, hipMemcpyDeviceToDevice, c->stream));
      HIPC(hipMemcpyAsync(c->imgqp_all.p + pplane * i, ent[i]->qp.p, pplane * 4, hipMemcpyDeviceToDevice, c->stream));
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
  const int cls = c->img_cls = pass_class(W, H, N, view_cls);
  DevBufs& B = c->bufs;
  if (cls != IMG_F32) TRY(bind_packed_arrays(c, cls, W, H, N));
  for (int i = 0; i < N; ++i) {
    HIPC(c->img_plain[i].ensure(L));
    HIPC(hipMemcpyAsync(c->img_plain[i].p, in->images[i], L * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (cls != IMG_F32) {
      TRY(build_packed_layouts(c->stream, c->img_plain[i].p, W, H, cls == IMG_U8 ? c->imgq8_all.p + plane * i : nullptr,
                               c->imgq16_all.p + plane * i, c->imgqp_all.p + pplane * i));
    } else {
      HIPC(c->imgq[i].ensure(plane));
      TRY(build_f32_quads(c->stream, c->img_plain[i].p, W, H, c->imgq[i].p));
      B.imgq[i] = c->imgq[i].p;
    }
  }
  B.ref = c->img_plain[0].p;
  return DPE_OK;
}

// Source depth maps of the geometric term: from the host, or the resident states (or their Jacobi
// snapshots) rescaled on the device.
static int stage_source_depths(DpeContext* c, const DpePassInput* in, const StageSrc& src) {
  const int W = in->width, H = in->height;
  const size_t L = (size_t)W * H;
  const dim3 rb2(32, 8), rg2((W + 31) / 32, (H + 7) / 8);
  for (int i = 1; i < in->num_images; ++i) {
    HIPC(c->depth[i].ensure(L));
    if (src.st) {
      HIPC(hipMemcpyAsync(c->depth[i].p, in->depths[i], L * sizeof(float), hipMemcpyHostToDevice, c->stream));
    } else {
      const ResState* r = src.dep[i];
      if (src.dep_snap)
        k_rescale_nearest<float><<<rg2, rb2, 0, c->stream>>>(r->snap.p, r->snap_w, r->snap_h, c->depth[i].p, W, H, 0.0f);
      else
        k_rescale_depth<<<rg2, rb2, 0, c->stream>>>(r->planes.p, r->w, r->h, c->depth[i].p, W, H);
      HIPC(hipGetLastError());
    }
    c->bufs.depth[i] = c->depth[i].p;
  }
  return DPE_OK;
}

static int stage_edge_label_maps(DpeContext* c, const DpePassInput* in) {
  const size_t L = (size_t)in->width * in->height, LL = (size_t)in->low_width * in->low_height;
  DevBufs& B = c->bufs;
  if (in->params.use_edge || in->params.use_limit) {
    HIPC(c->edge.ensure(L));
    HIPC(c->edge_low.ensure(LL));
    HIPC(hipMemcpyAsync(c->edge.p, in->edge, L, hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(c->edge_low.p, in->edge_low_res, LL, hipMemcpyHostToDevice, c->stream));
    B.edge = c->edge.p; B.edge_low = c->edge_low.p;
  }
  if (in->params.use_label) {
    HIPC(c->label.ensure(L));
    HIPC(hipMemcpyAsync(c->label.p, in->label, L * sizeof(int), hipMemcpyHostToDevice, c->stream));
    B.label = c->label.p;
  }
  return DPE_OK;
}

// The staged initial state (k_pass_init copies it at the start of every execute): from the host, or
// InuputInitialization's prior (DPE.cpp:845-911) from the resident state, rescaled on the device.
static int stage_initial_state(DpeContext* c, const DpePassInput* in, const StageSrc& src) {
  const DpePatchMatchParams& P = in->params;
  const int W = in->width, H = in->height;
  const size_t L = (size_t)W * H;
  HIPC(c->planes0.ensure(L)); HIPC(c->weak0.ensure(L)); HIPC(c->sel0.ensure(L));
  if (const DpePassState* st = src.st) {
    HIPC(hipMemcpyAsync(c->planes0.p, st->planes, L * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    if (P.use_APD) HIPC(hipMemcpyAsync(c->weak0.p, st->weak_info, L, hipMemcpyHostToDevice, c->stream));
    else HIPC(hipMemsetAsync(c->weak0.p, DPE_STRONG, L, c->stream));   // DPE.cpp:873-881
    HIPC(hipMemcpyAsync(c->sel0.p, st->selected_views, L * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    return DPE_OK;
  }
  const ResState* r = src.prior;
  const dim3 rb2(32, 8), rg2((W + 31) / 32, (H + 7) / 8);
  if (P.state != DPE_FIRST_INIT) {
    k_rescale_nearest<float4><<<rg2, rb2, 0, c->stream>>>(r->planes.p, r->w, r->h, c->planes0.p, W, H, make_float4(0, 0, 0, 0));
    k_rescale_nearest<uint32_t><<<rg2, rb2, 0, c->stream>>>(r->sel.p, r->w, r->h, c->sel0.p, W, H, 0u);
  } else {
    HIPC(hipMemsetAsync(c->planes0.p, 0, L * sizeof(float4), c->stream));
    HIPC(hipMemsetAsync(c->sel0.p, 0, L * sizeof(uint32_t), c->stream));
  }
  if (P.use_APD) k_rescale_nearest<uint8_t><<<rg2, rb2, 0, c->stream>>>(r->weak.p, r->w, r->h, c->weak0.p, W, H, (uint8_t)0);
  else HIPC(hipMemsetAsync(c->weak0.p, DPE_STRONG, L, c->stream));
  HIPC(hipGetLastError());
  return DPE_OK;
}

// The buffers a pass works in, sized for W x H and bound into the pass's DevBufs.
static int ensure_working_set(DpeContext* c, int W, int H) {
  const size_t L = (size_t)W * H;
  HIPC(c->planes.ensure(L)); HIPC(c->planes_snap.ensure(L)); HIPC(c->fit_plane.ensure(L));
  HIPC(c->costs.ensure(L)); HIPC(c->costs_snap.ensure(L)); HIPC(c->complex_.ensure(L));
  HIPC(c->sel.ensure(L)); HIPC(c->sel_snap.ensure(L));
  HIPC(c->weak.ensure(L)); HIPC(c->weak_rel.ensure(L)); HIPC(c->vw.ensure(L * DPE_MAX_IMAGES));
  HIPC(c->nb.ensure(L * 9)); HIPC(c->nearest.ensure(L)); HIPC(c->edge_neigh.ensure(L * 8)); HIPC(c->lab_bound.ensure(L * 8));
  HIPC(c->radius.ensure(L));
  HIPC(c->tab_right.ensure(L)); HIPC(c->tab_down.ensure(L));
  HIPC(c->gn_ovf.ensure(L + 64)); HIPC(c->gn_tab.ensure((size_t)W + H));
  const PassLists lay(W, H, c->hc.half_rows);   // the layout dpe_pm_execute carves them by (pass_lists.h)
  HIPC(c->lists.ensure((size_t)lay.lists_len())); HIPC(c->row_counts.ensure(lay.row_counts_len()));
  HIPC(c->list_totals.ensure(PassLists::kTotals)); HIPC(c->part_cnt.ensure(lay.part_cnt_len()));
  DevBufs& B = c->bufs;
  B.planes = c->planes.p; B.planes_snap = c->planes_snap.p; B.fit_plane = c->fit_plane.p;
  B.planes0 = c->planes0.p;
  B.costs = c->costs.p; B.costs_snap = c->costs_snap.p; B.complex_ = c->complex_.p;
  B.sel = c->sel.p; B.sel_snap = c->sel_snap.p;
  B.weak = c->weak.p; B.weak_rel = c->weak_rel.p; B.vw = c->vw.p;
  B.nb = c->nb.p; B.nearest = c->nearest.p; B.edge_neigh = c->edge_neigh.p; B.lab_bound = c->lab_bound.p;
  B.radius = c->radius.p;
  return DPE_OK;
}

static int stage_impl(DpeContext* c, const DpePassInput* in, const StageSrc& src) {
  Range range_(src.st ? "dpe_pm_stage" : "dpe_pm_stage_resident");
  TRY(stage_check_args(in));
  HIPC(hipSetDevice(c->device));
  HIPC(wait_pending(c));   // an earlier execute on a caller stream may still read what is overwritten here
  set_pass_constants(c->hc, in);
  HIPC(c->dc.ensure(1));
  HIPC(hipMemcpyAsync(c->dc.p, &c->hc, sizeof(PassConst), hipMemcpyHostToDevice, c->stream));
  std::memset(&c->bufs, 0, sizeof(c->bufs));
  TRY(in->image_ids ? stage_images_cached(c, in) : stage_images_direct(c, in));
  if (in->params.geom_consistency) TRY(stage_source_depths(c, in, src));
  TRY(stage_edge_label_maps(c, in));
  TRY(stage_initial_state(c, in, src));
  TRY(ensure_working_set(c, in->width, in->height));
  HIPC(hipStreamSynchronize(c->stream));
  c->staged = true;
#if DPE_GN_ONCE
  c->gn_done_for_stage = false;
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
    timing = c->timing;
#if DPE_PHASE_PROF
    HIPC(c->phase.ensure(32 * 64));
    HIPC(hipMemsetAsync(c->phase.p, 0, 32 * 64 * sizeof(unsigned long long), s));
    B.phase = c->phase.p;
#endif
    if (c->counting) {
      HIPC(c->cnt.ensure(DPE_NUM_CLASSES * 4));
      HIPC(hipMemsetAsync(c->cnt.p, 0, DPE_NUM_CLASSES * 4 * sizeof(unsigned long long), s));
    }
    max_slots = 5 + 5 * std::max(0, c->hc.P.max_iterations);
    while (timing && (int)c->ev.size() < 2 * max_slots) {
      Event e;
      HIPC(e.create(hipEventDefault));
      c->ev.push_back(std::move(e));
    }
    ev_class.assign(timing ? max_slots : 0, 0);
    for (int k = 0; k <= DPE_NUM_CLASSES; ++k) c->launches[k] = 0;
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
      if (r.c->counting) B.cnt = r.c->cnt.p + 4 * cls;
      r.c->launches[cls]++;
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
      for (int k = 0; k <= DPE_NUM_CLASSES; ++k) c->timings[k] = 0.0f;
      float ms = 0;
      (void)hipEventElapsedTime(&ms, c->ev_start, c->ev[2 * nev - 1]);
      c->timings[0] = ms;
      for (int e = 0; e < nev; ++e) {
        (void)hipEventElapsedTime(&ms, c->ev[2 * e], c->ev[2 * e + 1]);
        c->timings[1 + ev_class[e]] += ms;
      }
    }
#if DPE_PHASE_PROF
    unsigned long long ph32[32 * 64], ph[64] = {};
    HIPC(hipMemcpyAsync(ph32, c->phase.p, sizeof(ph32), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    for (int k = 0; k < 32 * 64; ++k) ph[k % 64] += ph32[k];
    unsigned long long tot[4] = {0, 0, 0, 0};
    for (int k = 0; k < 64; ++k) tot[k / 16] += ph[k];
    for (int k = 0; k < 64; ++k)
      if (ph[k]) fprintf(stderr, "PHASE %d.%d %.4e cycles %.1f%%\n", k / 16, k % 16, (double)ph[k], 100.0 * ph[k] / tot[k / 16]);
#endif
    if (c->counting) {
      HIPC(hipMemcpyAsync(c->counts, c->cnt.p, sizeof(c->counts), hipMemcpyDeviceToHost, s));
      HIPC(hipStreamSynchronize(s));
      for (int k = 0; k < DPE_NUM_CLASSES; ++k) c->counts[4 * k + 3] = (unsigned long long)c->launches[k];
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
      : c(c_), s(s_), a(s_), pc(c_->hc), dpc(c_->dc.p), B(c_->bufs), lay(pc.W, pc.H, pc.half_rows),
        L((size_t)pc.W * pc.H), nv(pc.N - 1) {
    static const bool overlap_env = [] { const char* e = getenv("DPE_OVERLAP"); return !(e && atoi(e) == 0); }();   // once per process
    overlap = overlap_env && !c->timing && !c->counting && pc.P.max_iterations >= 1;
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

  int* list(PassLists::Region r) const { return c->lists.p + r.off; }
  int* rows(PassLists::Region r) const { return c->row_counts.p + r.off; }
  int* total(int slot) const { return c->list_totals.p + slot; }
  int* chunk_counts(int colour) const { return c->part_cnt.p + lay.chunk_counts(colour).off; }
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
  if (X.gn_skip) {
  } else if (X.pc.P.rotate_time <= 4) {
    // the scratch-free kernel; pixels with more support points than its LDS slots (none at the
    // BASELINE workloads) or a NaN go to the scratch kernel, a small persistent grid that loops over
    // that overflow list (its count: the GenNeighbours-overflow total, dpe_pm_last_stat)
    int* ovf = X.total(PassLists::kTotGnOverflow);
    k_gn_tables<<<(unsigned)((X.pc.W + X.pc.H + 255) / 256), 256, 0, a>>>(X.dpc, c->gn_tab.p);
    HIPC(hipMemsetAsync(ovf, 0, sizeof(int), a));
    const unsigned gg = (unsigned)((X.L + kGnBT - 1) / kGnBT);
    if (c->gn_slots == 8)   // test setting: most pixels overflow into the scratch kernel
      k_gen_neighbours_lds<8><<<gg, kGnBT, 0, a>>>(X.dpc, Bc, weak_list, cnt, c->gn_tab.p, c->gn_ovf.p, ovf);
    else if (X.pc.P.rotate_time <= 2 && c->gn_slots != 64)   // at most 16 x rotate_time support points
      k_gen_neighbours_lds<32><<<gg, kGnBT, 0, a>>>(X.dpc, Bc, weak_list, cnt, c->gn_tab.p, c->gn_ovf.p, ovf);
    else
      k_gen_neighbours_lds<64><<<gg, kGnBT, 0, a>>>(X.dpc, Bc, weak_list, cnt, c->gn_tab.p, c->gn_ovf.p, ovf);
    k_gen_neighbours<<<kGnOvfBlocks, 256, 0, a>>>(X.dpc, Bc, c->gn_ovf.p, ovf);
  } else {
    k_gen_neighbours<<<kGnOvfBlocks, 256, 0, a>>>(X.dpc, Bc, weak_list, cnt);
  }
#if DPE_GN_ONCE
  if (!X.gn_skip) {   // kept for the next executes of this staged state (see dpe_pm_execute)
    HIPC(c->gn_complex.ensure(X.L));
    HIPC(hipMemcpyAsync(c->gn_complex.p, X.B.complex_, X.L * sizeof(float), hipMemcpyDeviceToDevice, a));
    c->gn_done_for_stage = true;
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
  if (X.gn_skip) HIPC(hipMemcpyAsync(X.B.complex_, c->gn_complex.p, X.L * sizeof(float), hipMemcpyDeviceToDevice, a));
#endif
  HIPC(X.aux_done(c->ev_ei));
  k_strong_tables_scan<<<(unsigned)(pc.W + pc.H), 64, 0, a>>>(X.dpc, Bc, c->tab_right.p, c->tab_down.p);
  k_find_nearest_strong<<<X.px_grid(), kPxBlock, 0, a>>>(X.dpc, Bc, c->tab_right.p, c->tab_down.p);
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
    if (X.c->img_cls != IMG_F32) k_random_init<kTexInit><<<X.px_grid(), kPxBlock, 0, X.s>>>(X.dpc, sec.B);
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
  launch_strong(edge, X.c->img_cls, grid, lds, X.s, X.dpc, Bs, it, X.list(list), X.total(total));
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
  if (X.c->img_cls == IMG_U8) k_weak_coop<kTexWeak, C><<<grid, 64 * wpb, per_wave * wpb, st>>>(X.dpc, Bc, it, lst, cnt);
  else if (X.c->img_cls == IMG_Q) k_weak_coop<TEX_F16, C><<<grid, 64 * wpb, per_wave * wpb, st>>>(X.dpc, Bc, it, lst, cnt);
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
    launch_local_refine(c->img_cls, (long)X.L, X.pc.W, X.pc.H, X.nv, st, X.dpc, sec.B);
  };
  HIPC(X.fork(c->ev_fork));
  if (X.overlap) border_local_refine(X.a);
  HIPC(X.aux_done(c->ev_join));
  {
    Section sec(X.rec, DPE_CLASS_DEPTH_TO_WEAK);
    launch_depth_to_weak(c->img_cls, (long)X.L, X.s, X.dpc, sec.B);
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
  ~GnGuard() { if (!ok) c->gn_done_for_stage = false; }
};
#endif

extern "C" int dpe_pm_execute(DpeContext* c, void* stream_) {
  TRY(enter(c, true, "dpe_pm_execute: null context"));
  if (!c->staged) { g_err = "dpe_pm_execute: call dpe_pm_stage first"; return DPE_ERR_STATE; }
  Range range_("dpe_pm_execute");
  hipStream_t s;
  // a previous execute, possibly on another stream, still uses the working buffers this one resets
  HIPC(enqueue_stream(c, stream_, &s));
  PassRun X(c, s);
  TRY(X.rec.start(c, s, X.B));
#if DPE_GN_ONCE
  X.gn_skip = c->gn_done_for_stage;
  GnGuard gn_guard{c};
#endif
  // initial state (the reference uploads it in CudaSpaceInitialization, DPE.cpp:964-1015); the rest
  // of it is cleared by the setup chain
  k_pass_init<<<(unsigned)((X.L + 255) / 256), 256, 0, s>>>((const uint4*)c->planes0.p, c->weak0.p, c->sel0.p, (uint4*)X.B.planes,
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
  if (!c->staged) { g_err = "dpe_pm_fetch: nothing staged"; return DPE_ERR_STATE; }
  Range range_("dpe_pm_fetch");
  const size_t L = (size_t)c->hc.W * c->hc.H;
  HIPC(host_wait(c));
  if (st->planes) HIPC(hipMemcpy(st->planes, c->bufs.planes, L * sizeof(float4), hipMemcpyDeviceToHost));
  if (st->weak_info) HIPC(hipMemcpy(st->weak_info, c->bufs.weak, L, hipMemcpyDeviceToHost));
  if (st->selected_views) HIPC(hipMemcpy(st->selected_views, c->bufs.sel, L * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (st->costs) HIPC(hipMemcpy(st->costs, c->bufs.costs, L * sizeof(float), hipMemcpyDeviceToHost));
  return DPE_OK;
}

extern "C" int dpe_pm_run(DpeContext* c, const DpePassInput* in, const DpePassState* st) {
  int r = dpe_pm_stage(c, in, st);
  if (r) return r;
  r = dpe_pm_execute(c, nullptr);
  if (r) return r;
  return dpe_pm_fetch(c, st);
}

extern "C" void* dpe_pm_device_planes(DpeContext* c) { return (c && c->staged) ? (void*)c->bufs.planes : nullptr; }

__global__ void k_export_depth(const float4* __restrict__ p, float* __restrict__ d, size_t L) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < L) d[i] = p[i].w;
}

extern "C" int dpe_pm_export_depth(DpeContext* c, float* dev_dst, void* stream_) {
  TRY(enter(c, dev_dst != nullptr, "dpe_pm_export_depth: null argument"));
  if (!c->staged) { g_err = "dpe_pm_export_depth: nothing staged"; return DPE_ERR_STATE; }
  hipStream_t s;
  HIPC(enqueue_stream(c, stream_, &s));   // after the pass that writes the planes
  const size_t L = (size_t)c->hc.W * c->hc.H;
  k_export_depth<<<(unsigned)((L + 255) / 256), 256, 0, s>>>(c->bufs.planes, dev_dst, L);
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
  if (!c->staged) { g_err = "dpe_state_save: nothing staged"; return DPE_ERR_STATE; }
  Range range_("dpe_state_save");
  const int W = c->hc.W, H = c->hc.H;
  const size_t L = (size_t)W * H;
  hipStream_t s;
  HIPC(enqueue_stream(c, nullptr, &s));   // the context's stream, after the pass that wrote the outputs
  ResState* r = &c->rstore[image_id];
  HIPC(r->planes.ensure(L)); HIPC(r->weak.ensure(L)); HIPC(r->sel.ensure(L));
  r->w = W; r->h = H; r->full = true;
  k_state_save<<<(unsigned)((L + 255) / 256), 256, 0, s>>>(c->bufs.planes, c->bufs.weak, c->bufs.sel, c->hc.P.depth_min,
                                                          c->hc.P.depth_max, r->planes.p, r->weak.p, r->sel.p, L);
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

// ------------------------------------------------------------------------------ EdgeSegment stages
namespace {
// cv::resize INTER_LINEAR CV_32F taps (host/hostio.cpp linear_taps)
void f32_taps(int n_src, int n_dst, int* s0, int* s1, float* a0, float* a1) {
  const double scale = 1.0 / ((double)n_dst / n_src);
  for (int d = 0; d < n_dst; ++d) {
    float f = (float)((d + 0.5) * scale - 0.5);
    int sidx = (int)std::floor(f);
    f -= (float)sidx;
    if (sidx < 0) { f = 0; sidx = 0; }
    if (sidx >= n_src - 1) { f = 0; sidx = n_src - 1; }
    s0[d] = sidx; s1[d] = std::min(sidx + 1, n_src - 1);
    a0[d] = 1.0f - f; a1[d] = f;
  }
}
// cv::resize INTER_LINEAR CV_8U taps (host/edges.cpp lin_tab): 11-bit weights, cvRound half to even
int u8_taps(int ssize, int dsize, int* ofs, short* a) {
  const double scale = 1.0 / ((double)dsize / ssize);
  int xmax = dsize;
  for (int d = 0; d < dsize; ++d) {
    float f = (float)((d + 0.5) * scale - 0.5);
    int sidx = (int)std::floor(f);
    f -= (float)sidx;
    if (sidx < 0) { f = 0; sidx = 0; }
    if (sidx + 1 >= ssize) {
      xmax = std::min(xmax, d);
      if (sidx >= ssize - 1) { f = 0; sidx = ssize - 1; }
    }
    ofs[d] = sidx;
    const float c0 = 1.0f - f, c1 = f;
    a[2 * d] = (short)std::min(32767, std::max(-32768, (int)std::nearbyint(c0 * 2048.0f)));
    a[2 * d + 1] = (short)std::min(32767, std::max(-32768, (int)std::nearbyint(c1 * 2048.0f)));
  }
  return xmax;
}
}  // namespace

extern "C" int dpe_resize_linear(DpeContext* c, const float* src, int w, int h, float* dst, int nw, int nh) {
  TRY(enter(c, src && dst && w >= 1 && h >= 1 && nw >= 1 && nh >= 1, "dpe_resize_linear: bad argument"));
  if (w == nw && h == nh) { std::memcpy(dst, src, sizeof(float) * (size_t)w * h); return DPE_OK; }
  std::vector<int> it(2 * (size_t)(nw + nh));
  std::vector<float> ft(2 * (size_t)(nw + nh));
  f32_taps(w, nw, it.data(), it.data() + nw, ft.data(), ft.data() + nw);
  f32_taps(h, nh, it.data() + 2 * nw, it.data() + 2 * nw + nh, ft.data() + 2 * nw, ft.data() + 2 * nw + nh);
  HIPC(c->e_fa.ensure((size_t)w * h)); HIPC(c->e_fb.ensure((size_t)nw * nh));
  HIPC(c->e_rows.ensure((size_t)h * nw));   // f32 rows stored in the int scratch (same size)
  HIPC(c->e_itab.ensure(it.size())); HIPC(c->e_ftab.ensure(ft.size()));
  HIPC(hipMemcpyAsync(c->e_fa.p, src, sizeof(float) * (size_t)w * h, hipMemcpyHostToDevice, c->stream));
  HIPC(hipMemcpyAsync(c->e_itab.p, it.data(), it.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPC(hipMemcpyAsync(c->e_ftab.p, ft.data(), ft.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  float* rows = (float*)c->e_rows.p;
  const dim3 b(32, 8);
  k_resize_linear_h<<<dim3((nw + 31) / 32, (h + 7) / 8), b, 0, c->stream>>>(c->e_fa.p, w, h, c->e_itab.p, c->e_itab.p + nw,
                                                                            c->e_ftab.p, c->e_ftab.p + nw, rows, nw);
  k_resize_linear_v<<<dim3((nw + 31) / 32, (nh + 7) / 8), b, 0, c->stream>>>(rows, nw, c->e_itab.p + 2 * nw,
                                                                             c->e_itab.p + 2 * nw + nh, c->e_ftab.p + 2 * nw,
                                                                             c->e_ftab.p + 2 * nw + nh, c->e_fb.p, nh);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(dst, c->e_fb.p, sizeof(float) * (size_t)nw * nh, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  return DPE_OK;
}

// device-to-device core of dpe_resize_u8 (src / dst in the context's scratch)
static int resize_u8_dev(DpeContext* c, const uint8_t* dsrc, int w, int h, uint8_t* ddst, int nw, int nh) {
  const dim3 b(32, 8);
  if (w == nw && h == nh) { HIPC(hipMemcpyAsync(ddst, dsrc, (size_t)w * h, hipMemcpyDeviceToDevice, c->stream)); return DPE_OK; }
  const double scale_x = 1.0 / ((double)nw / w), scale_y = 1.0 / ((double)nh / h);
  const int isx = (int)std::lround(scale_x), isy = (int)std::lround(scale_y);
  const bool area_fast = std::fabs(scale_x - isx) < 2.220446049250313e-16 && std::fabs(scale_y - isy) < 2.220446049250313e-16;
  if (area_fast && isx == 2 && isy == 2) {   // INTER_LINEAR at exactly 1/2 = INTER_AREA's fast path
    k_resize_u8_half<<<dim3((nw + 31) / 32, (nh + 7) / 8), b, 0, c->stream>>>(dsrc, w, ddst, nw, nh);
    HIPC(hipGetLastError());
    return DPE_OK;
  }
  std::vector<int> ofs((size_t)nw + nh);
  std::vector<short> a(2 * ((size_t)nw + nh));
  const int xmax = u8_taps(w, nw, ofs.data(), a.data());
  (void)u8_taps(h, nh, ofs.data() + nw, a.data() + 2 * nw);
  int xv = 0;                                 // VResizeLinear: 16-lane, then 8-lane vector blocks
  for (; xv <= nw - 16; xv += 16) {}
  for (; xv < nw - 8; xv += 8) {}
  HIPC(c->e_rows.ensure((size_t)h * nw)); HIPC(c->e_itab.ensure(ofs.size())); HIPC(c->e_stab.ensure(a.size()));
  HIPC(hipMemcpyAsync(c->e_itab.p, ofs.data(), ofs.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPC(hipMemcpyAsync(c->e_stab.p, a.data(), a.size() * sizeof(short), hipMemcpyHostToDevice, c->stream));
  k_resize_u8_h<<<dim3((nw + 31) / 32, (h + 7) / 8), b, 0, c->stream>>>(dsrc, w, h, c->e_itab.p, c->e_stab.p, xmax,
                                                                        c->e_rows.p, nw);
  k_resize_u8_v<<<dim3((nw + 31) / 32, (nh + 7) / 8), b, 0, c->stream>>>(c->e_rows.p, h, nw, c->e_itab.p + nw,
                                                                         c->e_stab.p + 2 * nw, xv, ddst, nh);
  HIPC(hipGetLastError());
  return DPE_OK;
}

extern "C" int dpe_resize_u8(DpeContext* c, const uint8_t* src, int w, int h, uint8_t* dst, int nw, int nh) {
  TRY(enter(c, src && dst && w >= 1 && h >= 1 && nw >= 1 && nh >= 1, "dpe_resize_u8: bad argument"));
  HIPC(c->e_a.ensure((size_t)w * h)); HIPC(c->e_b.ensure((size_t)nw * nh));
  HIPC(hipMemcpyAsync(c->e_a.p, src, (size_t)w * h, hipMemcpyHostToDevice, c->stream));
  TRY(resize_u8_dev(c, c->e_a.p, w, h, c->e_b.p, nw, nh));
  HIPC(hipMemcpyAsync(dst, c->e_b.p, (size_t)nw * nh, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  return DPE_OK;
}

extern "C" int dpe_roberts_threshold(DpeContext* c, const uint8_t* src, int w, int h, int thr, uint8_t* dst) {
  TRY(enter(c, src && dst && w >= 1 && h >= 1, "dpe_roberts_threshold: bad argument"));
  HIPC(c->e_a.ensure((size_t)w * h)); HIPC(c->e_b.ensure((size_t)w * h));
  HIPC(hipMemcpyAsync(c->e_a.p, src, (size_t)w * h, hipMemcpyHostToDevice, c->stream));
  k_roberts_threshold<<<dim3((w + 31) / 32, (h + 7) / 8), dim3(32, 8), 0, c->stream>>>(c->e_a.p, w, h, thr, c->e_b.p);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(dst, c->e_b.p, (size_t)w * h, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  return DPE_OK;
}

extern "C" int dpe_canny(DpeContext* c, const uint8_t* src, int w, int h, double low_thresh, double high_thresh, uint8_t* dst) {
  TRY(enter(c, src && dst && w >= 1 && h >= 1, "dpe_canny: bad argument"));
  Range range_("dpe_canny");
  if (low_thresh > high_thresh) std::swap(low_thresh, high_thresh);   // canny.cpp threshold handling
  low_thresh = std::min(32767.0, low_thresh);
  high_thresh = std::min(32767.0, high_thresh);
  if (low_thresh > 0) low_thresh *= low_thresh;
  if (high_thresh > 0) high_thresh *= high_thresh;
  const int low = (int)std::floor(low_thresh), high = (int)std::floor(high_thresh);
  const int ms = w + 2;
  const size_t L = (size_t)w * h, M = (size_t)ms * (h + 2);
  HIPC(c->e_a.ensure(L)); HIPC(c->e_dx.ensure(L)); HIPC(c->e_dy.ensure(L)); HIPC(c->e_mag.ensure(M)); HIPC(c->e_map.ensure(M));
  HIPC(hipMemcpyAsync(c->e_a.p, src, L, hipMemcpyHostToDevice, c->stream));
  const dim3 b(32, 8), g((ms + 31) / 32, (h + 2 + 7) / 8);
  k_canny_sobel<<<g, b, 0, c->stream>>>(c->e_a.p, w, h, c->e_dx.p, c->e_dy.p, c->e_mag.p);
  k_canny_nms<<<g, b, 0, c->stream>>>(c->e_dx.p, c->e_dy.p, c->e_mag.p, w, h, low, high, c->e_map.p);
  HIPC(hipGetLastError());
  std::vector<uint8_t> map(M);
  HIPC(hipMemcpyAsync(map.data(), c->e_map.p, M, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  // hysteresis: 8-connected growth through candidates from every strong candidate (any order: the
  // closure is the same set)
  std::vector<size_t> stack;
  stack.reserve(L / 8 + 16);
  for (size_t i = 0; i < M; ++i) if (map[i] == 2) stack.push_back(i);
  const long off[8] = {-ms - 1, -ms, -ms + 1, -1, 1, ms - 1, ms, ms + 1};
  while (!stack.empty()) {
    const size_t i = stack.back();
    stack.pop_back();
    for (long o : off) {
      const size_t j = (size_t)((long)i + o);
      if (!map[j]) { map[j] = 2; stack.push_back(j); }
    }
  }
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) dst[(size_t)y * w + x] = map[(size_t)(y + 1) * ms + x + 1] == 2 ? 255 : 0;
  return DPE_OK;
}

extern "C" void dpe_state_clear(DpeContext* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)host_wait(c);
  c->rstore.clear();
  c->snap_mode = false;
#if DPE_GN_ONCE
  c->gn_done_for_stage = false;
#endif
}

extern "C" int dpe_host_pin(void* ptr, size_t bytes) {
  if (!ptr || bytes == 0) return DPE_ERR_ARG;
  return hipHostRegister(ptr, bytes, hipHostRegisterDefault) == hipSuccess ? DPE_OK : DPE_ERR_HIP;
}
extern "C" int dpe_host_unpin(void* ptr) {
  if (!ptr) return DPE_ERR_ARG;
  return hipHostUnregister(ptr) == hipSuccess ? DPE_OK : DPE_ERR_HIP;
}

// ---------------------------------------------------------------- viz medium results (pass_viz.h)
static std::atomic<long long> g_viz_launches{0};

extern "C" long long dpe_viz_launches(void) { return g_viz_launches.load(); }

static size_t viz_block_values(int w, int h) { return (size_t)((w + 15) / 16) * ((h + 15) / 16) * 6 * 64; }

// the picture of (planes, weak) into c->viz_bgr on stream s
static int viz_enqueue_render(DpeContext* c, int kind, const float4* planes, const uint8_t* weak, int w, int h, float dmin,
                              float dmax, hipStream_t s) {
  const size_t L = (size_t)w * h;
  HIPC(c->viz_bgr.ensure(3 * L));
  k_viz_render<<<(unsigned)((L + 1023) / 1024), 256, 0, s>>>(kind, planes, weak, dmin, dmax, c->viz_bgr.p, L);
  HIPC(hipGetLastError());
  g_viz_launches++;
  return DPE_OK;
}

// the JPEG front half of c->viz_bgr (w x h) into c->viz_blocks on stream s
static int viz_enqueue_front(DpeContext* c, int w, int h, int quality, hipStream_t s) {
  if (c->viz_quality != quality) {   // first use, or another quality: no kernel may still read the old tables
    HIPC(hipStreamSynchronize(s));
    HIPC(hipStreamSynchronize(c->stream));
    uint16_t q[128];
    dpe_jpeg::quant_tables(quality, q);
    HIPC(c->viz_q.ensure(128));
    HIPC(hipMemcpy(c->viz_q.p, q, sizeof(q), hipMemcpyHostToDevice));
    c->viz_quality = quality;
  }
  HIPC(c->viz_blocks.ensure(viz_block_values(w, h)));
  k_jpeg_front<<<dim3((unsigned)((w + 15) / 16), (unsigned)((h + 15) / 16)), 384, 0, s>>>(c->viz_bgr.p, w, h, c->viz_q.p,
                                                                                        c->viz_blocks.p);
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
  HIPC(hipMemcpyAsync(host_bgr, c->viz_bgr.p, (size_t)r->w * r->h * 3, hipMemcpyDeviceToHost, s));
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
  HIPC(hipMemcpyAsync(host_blocks, c->viz_blocks.p, n * sizeof(int16_t), hipMemcpyDeviceToHost, s));
  hipEvent_t ev = nullptr;
  {
    std::lock_guard<std::mutex> lk(c->viz_mu);
    auto it = c->viz_ev.find(host_blocks);
    if (it == c->viz_ev.end()) {
      Event fresh;
      HIPC(fresh.create());
      it = c->viz_ev.emplace(host_blocks, std::move(fresh)).first;
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
    std::lock_guard<std::mutex> lk(c->viz_mu);
    auto it = c->viz_ev.find(host_blocks);
    if (it == c->viz_ev.end()) { g_err = "dpe_state_render_wait: no render into this buffer"; return DPE_ERR_ARG; }
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
  HIPC(c->viz_planes.ensure(L));
  HIPC(c->viz_weak.ensure(L));
  HIPC(hipMemcpy(c->viz_planes.p, p.data(), L * sizeof(float4), hipMemcpyHostToDevice));
  if (weak) HIPC(hipMemcpy(c->viz_weak.p, weak, L, hipMemcpyHostToDevice));
  else HIPC(hipMemset(c->viz_weak.p, 0, L));
  TRY(viz_enqueue_render(c, kind, c->viz_planes.p, c->viz_weak.p, w, h, dmin, dmax, c->stream));
  HIPC(hipMemcpyAsync(host_bgr, c->viz_bgr.p, 3 * L, hipMemcpyDeviceToHost, c->stream));
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
  HIPC(c->viz_bgr.ensure((size_t)w * h * 3));
  HIPC(hipMemcpy(c->viz_bgr.p, host_bgr, (size_t)w * h * 3, hipMemcpyHostToDevice));
  TRY(viz_enqueue_front(c, w, h, quality, c->stream));
  HIPC(hipMemcpyAsync(host_blocks, c->viz_blocks.p, n * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  return DPE_OK;
}

extern "C" int dpe_fusion_stage(DpeContext* c, const DpeFusionView* views, int n) {
  TRY(enter(c, views && n >= 1, "dpe_fusion_stage: bad argument"));
  c->tat_ready = false;   // the colours and masks of dpe_fusion_tat_begin belong to the views staged before
  c->fz_depth.resize(n); c->fz_normal.resize(n); c->fz_host.assign(n, FusionViewDev{});
  std::vector<DpeCamera> cams(n);
  for (int i = 0; i < n; ++i) {
    const DpeFusionView& v = views[i];
    if (v.width < 1 || v.height < 1 || !v.depth || !v.normal) { g_err = "dpe_fusion_stage: bad view"; return DPE_ERR_ARG; }
    const size_t L = (size_t)v.width * v.height;
    HIPC(c->fz_depth[i].ensure(L));
    HIPC(c->fz_normal[i].ensure(3 * L));
    HIPC(hipMemcpyAsync(c->fz_depth[i].p, v.depth, L * 4, hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(c->fz_normal[i].p, v.normal, 3 * L * 4, hipMemcpyHostToDevice, c->stream));
    c->fz_host[i] = FusionViewDev{c->fz_depth[i].p, c->fz_normal[i].p, v.width, v.height};
    cams[i] = v.cam;
  }
  HIPC(c->fz_views.ensure(n));
  HIPC(c->fz_cams.ensure(n));
  HIPC(hipMemcpyAsync(c->fz_views.p, c->fz_host.data(), n * sizeof(FusionViewDev), hipMemcpyHostToDevice, c->stream));
  HIPC(hipMemcpyAsync(c->fz_cams.p, cams.data(), n * sizeof(DpeCamera), hipMemcpyHostToDevice, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  c->fz_n = n;
  return DPE_OK;
}

extern "C" int dpe_fusion_candidates(DpeContext* c, int ref, const int* src, int ns, int32_t* idx, float* val) {
  TRY(enter(c, src && idx && val && ns >= 0, "dpe_fusion_candidates: bad argument"));
  if (c->fz_n < 1) { g_err = "dpe_fusion_candidates: nothing staged"; return DPE_ERR_STATE; }
  if (ref < 0 || ref >= c->fz_n) { g_err = "dpe_fusion_candidates: bad reference view"; return DPE_ERR_ARG; }
  for (int j = 0; j < ns; ++j)
    if (src[j] < 0 || src[j] >= c->fz_n) { g_err = "dpe_fusion_candidates: bad source view"; return DPE_ERR_ARG; }
  if (ns == 0) return DPE_OK;
  const size_t L = (size_t)c->fz_host[ref].w * c->fz_host[ref].h;
  HIPC(c->fz_src.ensure(ns));
  HIPC(c->fz_idx.ensure(L * ns));
  HIPC(c->fz_val.ensure(L * ns * 3));
  HIPC(hipMemcpyAsync(c->fz_src.p, src, ns * sizeof(int), hipMemcpyHostToDevice, c->stream));
  k_fusion_candidates<<<(unsigned)((L + 255) / 256), 256, 0, c->stream>>>(c->fz_cams.p, c->fz_views.p, ref, c->fz_src.p, ns,
                                                                         c->fz_idx.p, c->fz_val.p);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(idx, c->fz_idx.p, L * ns * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPC(hipMemcpyAsync(val, c->fz_val.p, L * ns * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  return DPE_OK;
}

// host-waits for the copy-out of the last dpe_fusion_tat_image
static hipError_t tat_wait_copy(DpeContext* c) {
  hipError_t e = hipSuccess;
  if (c->tat_copying) { e = hipEventSynchronize(c->ev_tat); c->tat_copying = false; }
  return e;
}

extern "C" int dpe_fusion_tat_begin(DpeContext* c, const uint8_t* const* bgr, const uint8_t* const* block) {
  TRY(enter(c, bgr != nullptr, "dpe_fusion_tat_begin: bad argument"));
  if (c->fz_n < 1) { g_err = "dpe_fusion_tat_begin: nothing staged"; return DPE_ERR_STATE; }
  const int n = c->fz_n;
  for (int i = 0; i < n; ++i)
    if (!bgr[i]) { g_err = "dpe_fusion_tat_begin: missing colour image"; return DPE_ERR_ARG; }
  HIPC(host_wait(c));
  HIPC(tat_wait_copy(c));
  c->tat_ready = false;
  c->tat_bgr.resize(n); c->tat_block.resize(n); c->tat_mask.resize(n);
  std::vector<TatViewDev> tv(n);
  for (int i = 0; i < n; ++i) {
    const size_t L = (size_t)c->fz_host[i].w * c->fz_host[i].h;
    HIPC(c->tat_bgr[i].ensure(3 * L));
    HIPC(c->tat_mask[i].ensure(L));
    HIPC(hipMemcpyAsync(c->tat_bgr[i].p, bgr[i], 3 * L, hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemsetAsync(c->tat_mask[i].p, 0, L, c->stream));
    const bool blk = block && block[i];
    if (blk) {
      HIPC(c->tat_block[i].ensure(L));
      HIPC(hipMemcpyAsync(c->tat_block[i].p, block[i], L, hipMemcpyHostToDevice, c->stream));
    }
    tv[i] = TatViewDev{c->tat_bgr[i].p, blk ? c->tat_block[i].p : nullptr, c->tat_mask[i].p};
  }
  HIPC(c->tat_views.ensure(n));
  HIPC(hipMemcpyAsync(c->tat_views.p, tv.data(), n * sizeof(TatViewDev), hipMemcpyHostToDevice, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  c->tat_ready = true;
  return DPE_OK;
}

extern "C" int dpe_fusion_tat_image(DpeContext* c, int mode, int ref, const int* src, int ns, const float* dot_thresholds,
                                    DpeFusedPoint* out, size_t cap, size_t* n_out) {
  static_assert(sizeof(DpeFusedPoint) == sizeof(TatPoint), "DpeFusedPoint layout");
  TRY(enter(c, n_out && ns >= 0 && (ns == 0 || src) && (out || cap == 0), "dpe_fusion_tat_image: bad argument"));
  if (!c->tat_ready) { g_err = "dpe_fusion_tat_image: dpe_fusion_tat_begin has not run"; return DPE_ERR_STATE; }
  if (mode != DPE_FUSION_TAT_INTERMEDIATE && mode != DPE_FUSION_TAT_ADVANCED) { g_err = "dpe_fusion_tat_image: bad mode"; return DPE_ERR_ARG; }
  if (ref < 0 || ref >= c->fz_n) { g_err = "dpe_fusion_tat_image: bad reference view"; return DPE_ERR_ARG; }
  if (ns > kTatMaxSrc) { g_err = "dpe_fusion_tat_image: more than 31 source views"; return DPE_ERR_TOO_MANY; }
  for (int j = 0; j < ns; ++j) {
    if (src[j] < 0 || src[j] >= c->fz_n) { g_err = "dpe_fusion_tat_image: bad source view"; return DPE_ERR_ARG; }
    // the kernels read the masks of the source views while they write the reference view's
    if (src[j] == ref) { g_err = "dpe_fusion_tat_image: the reference view is among its sources"; return DPE_ERR_ARG; }
  }
  if (mode == DPE_FUSION_TAT_INTERMEDIATE && ns >= 2 && !dot_thresholds) { g_err = "dpe_fusion_tat_image: no thresholds"; return DPE_ERR_ARG; }
  *n_out = 0;
  if (ns < 2) {   // the k loop starts at 2 (DPE.cpp:1504): no point, no mask
    HIPC(tat_wait_copy(c));
    return DPE_OK;
  }
  const size_t L = (size_t)c->fz_host[ref].w * c->fz_host[ref].h;
  const int nch = (int)((L + kTatChunk - 1) / kTatChunk);
  DevArr<TatPoint>& dout = c->tat_out[c->tat_turn];
  HIPC(c->fz_src.ensure(ns));
  HIPC(c->tat_dthr.ensure(kTatMaxSrc + 1));
  HIPC(c->tat_last.ensure(L * ns));
  HIPC(c->tat_agg.ensure((size_t)nch * ns));
  HIPC(c->tat_cnt.ensure(nch));
  HIPC(c->tat_tot.ensure(1));
  HIPC(c->tat_emit.ensure(L));
  HIPC(c->tat_rec.ensure(L));
  HIPC(dout.ensure(L));
  hipStream_t s;
  HIPC(enqueue_stream(c, nullptr, &s));
  float dthr[kTatMaxSrc + 1] = {0};
  if (mode == DPE_FUSION_TAT_INTERMEDIATE)
    for (int k = 2; k <= ns; ++k) dthr[k] = dot_thresholds[k];
  // (the stream is synchronised below, before `dthr` and the caller's `src` go out of scope)
  HIPC(hipMemcpyAsync(c->fz_src.p, src, ns * sizeof(int), hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(c->tat_dthr.p, dthr, sizeof(dthr), hipMemcpyHostToDevice, s));
  k_tat_hit_scan<<<nch, kTatChunk, 0, s>>>(c->fz_cams.p, c->fz_views.p, c->tat_views.p, ref, c->fz_src.p, ns, nch,
                                          c->tat_last.p, c->tat_agg.p);
  k_tat_chunk_carry<<<ns, 256, 0, s>>>(nch, c->tat_agg.p);
  k_tat_decide<<<nch, kTatChunk, 0, s>>>(c->fz_cams.p, c->fz_views.p, c->tat_views.p, ref, c->fz_src.p, ns, nch, mode,
                                        c->tat_dthr.p, c->tat_last.p, c->tat_agg.p, c->tat_rec.p, c->tat_emit.p,
                                        c->tat_cnt.p);
  k_tat_offsets<<<1, 256, 0, s>>>(nch, c->tat_cnt.p, c->tat_tot.p);
  k_tat_fill<<<nch, kTatChunk, 0, s>>>((int)L, c->tat_emit.p, c->tat_rec.p, c->tat_cnt.p, dout.p);
  HIPC(hipGetLastError());
  int total = 0;
  HIPC(hipMemcpyAsync(&total, c->tat_tot.p, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  HIPC(tat_wait_copy(c));   // the copy-out of the image before ran beside these kernels
  if (total < 0 || (size_t)total > L) { g_err = "dpe_fusion_tat_image: bad point count"; return DPE_ERR_STATE; }
  *n_out = (size_t)total;
  if ((size_t)total > cap) { g_err = "dpe_fusion_tat_image: output buffer too small"; return DPE_ERR_ARG; }
  if (total > 0) {
    HIPC(hipMemcpyAsync(out, dout.p, (size_t)total * sizeof(TatPoint), hipMemcpyDeviceToHost, c->aux));
    HIPC(hipEventRecord(c->ev_tat, c->aux));
    c->tat_copying = true;
    c->tat_turn ^= 1;
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
  if (!c->tat_ready) { g_err = "dpe_fusion_tat_mask: dpe_fusion_tat_begin has not run"; return DPE_ERR_STATE; }
  if (view < 0 || view >= c->fz_n) { g_err = "dpe_fusion_tat_mask: bad view"; return DPE_ERR_ARG; }
  HIPC(host_wait(c));
  HIPC(hipMemcpy(mask, c->tat_mask[view].p, (size_t)c->fz_host[view].w * c->fz_host[view].h, hipMemcpyDeviceToHost));
  return DPE_OK;
}

extern "C" int dpe_pm_last_timings(DpeContext* c, float* out, int n) {
  if (!c || !out) return 0;
  const int m = n < DPE_NUM_CLASSES + 1 ? n : DPE_NUM_CLASSES + 1;
  for (int i = 0; i < m; ++i) out[i] = c->timings[i];
  return m;
}

extern "C" void dpe_set_counting(DpeContext* c, int enable) { if (c) c->counting = enable != 0; }

extern "C" int dpe_set_option(DpeContext* c, int option, int value) {
  g_err.clear();   // (touches no device)
  if (!c) { g_err = "dpe_set_option: null context"; return DPE_ERR_ARG; }
  if (option == DPE_OPT_GN_SLOTS && (value == 0 || value == 8 || value == 32 || value == 64)) { c->gn_slots = value; return DPE_OK; }
  g_err = "dpe_set_option: unknown option or value";
  return DPE_ERR_ARG;
}

extern "C" long long dpe_pm_last_stat(DpeContext* c, int stat) {
  if (c && c->staged && stat == DPE_STAT_TEX_CLASS) return c->img_cls;
  if (!c || !c->staged || stat != DPE_STAT_GN_DEFERRED || !c->list_totals.p) return -1;
  int v = 0;   // waits for this context's pass only (not the whole device)
  if (hipSetDevice(c->device) != hipSuccess || wait_pending(c) != hipSuccess || hipStreamSynchronize(c->aux) != hipSuccess ||
      hipMemcpyAsync(&v, c->list_totals.p + PassLists::kTotGnOverflow, sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess)
    return -1;
  return v;
}

extern "C" int dpe_pm_last_counts(DpeContext* c, unsigned long long* out, int n) {
  if (!c || !out) return 0;
  const int m = n < DPE_NUM_CLASSES * 4 ? n : DPE_NUM_CLASSES * 4;
  for (int i = 0; i < m; ++i) out[i] = c->counts[i];
  return m;
}
