/*
 * dpe_mvs.h — C-ABI of the MI355X-native PatchMatch pass (the DPE-MVS hot path).
 *
 * This header is the drop-in boundary.  It replaces the inner seam of the reference's
 * per-image host object `class DPE`:
 *
 *   reference                                   replaced by
 *   ------------------------------------------  ------------------------------------------
 *   DPE::CudaSpaceInitialization  DPE.cpp:916   dpe_pm_stage()   (H2D, layout, workspaces)
 *   DPE::SetDataPassHelperInCuda  DPE.cpp:1054  (internal: device pointer bundle)
 *   DPE::RunPatchMatch            DPE.cu:3126   dpe_pm_execute() (the 26-launch pass)
 *   DPE::GetPlaneHypothesis       DPE.cpp:1091  dpe_pm_fetch()   (D2H of planes /
 *   DPE::GetPixelStates           DPE.cpp:1099                     weak_info / selected_views)
 *   DPE::GetSelectedViews         DPE.cpp:1103
 *   DPE::~DPE                     DPE.cpp:679   dpe_destroy()
 *   CudaSafeCall -> exit()        DPE.cpp:633   return codes + dpe_last_error()
 *
 * The caller (host orchestration, the reference's ProcessProblem main.cpp:411-446) keeps
 * doing InuputInitialization (DPE.cpp:733-914: image decode/resize, camera read, depth range
 * x0.6/x1.2, prior rescale) and the epilogue (main.cpp:427-446).
 *
 * Types are plain C: no torch, no HIP types.  `DpeCamera` and `DpePatchMatchParams` are
 * layout-compatible with the reference's `Camera` (main.h:50-59) and `PatchMatchParams`
 * (main.h:78-106); enum values match `RunState` / `PixelState` (main.h:66-76).
 */
#ifndef DPE_MVS_H_
#define DPE_MVS_H_

#include <stdint.h>
#include <stddef.h>
#ifndef __cplusplus
#include <stdbool.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define DPE_ABI_VERSION 1
#define DPE_MAX_IMAGES 32      /* main.h:40  MAX_IMAGES     */
#define DPE_NEIGHBOUR_NUM 9    /* main.h:41  NEIGHBOUR_NUM  */

/* main.h:66-70 RunState */
enum { DPE_FIRST_INIT = 0, DPE_REFINE_INIT = 1, DPE_REFINE_ITER = 2 };
/* main.h:72-76 PixelState */
enum { DPE_WEAK = 0, DPE_STRONG = 1, DPE_UNKNOWN = 2 };

/* Error codes (the reference exits the process instead, DPE.cpp:633-641, :762-765). */
enum {
  DPE_OK = 0,
  DPE_ERR_ARG = -1,       /* bad argument / shape */
  DPE_ERR_HIP = -2,       /* HIP runtime error */
  DPE_ERR_NOMEM = -3,     /* allocation failed */
  DPE_ERR_STATE = -4,     /* call order (execute before stage, ...) */
  DPE_ERR_TOO_MANY = -5   /* num_images > DPE_MAX_IMAGES (DPE.cpp:762) */
};

/* main.h:50-59 struct Camera (112 bytes) */
typedef struct DpeCamera {
  float K[9];
  float R[9];
  float t[3];
  float c[3];
  int height;
  int width;
  float depth_min;
  float depth_max;
} DpeCamera;

/* main.h:78-106 struct PatchMatchParams, same field order and C types. */
typedef struct DpePatchMatchParams {
  int max_iterations;     /* 3 */
  int num_images;         /* 1 ref + Ns src */
  float sigma_spatial;    /* 5 */
  float sigma_color;      /* 3 */
  int top_k;              /* 4 */
  float depth_min;
  float depth_max;
  bool geom_consistency;
  int strong_radius;      /* 5 */
  int strong_increment;   /* 2 */
  int weak_radius;        /* 5 */
  int weak_increment;     /* 5 */
  bool use_APD;
  bool use_edge;
  bool use_limit;
  bool use_label;
  bool use_radius;
  bool high_res_img;
  int max_scale_size;
  int scale_size;
  int weak_peak_radius;   /* 2 */
  int rotate_time;        /* 4 */
  float ransac_threshold; /* 0.005 */
  float geom_factor;      /* 0.2 */
  int state;              /* RunState */
} DpePatchMatchParams;

/* Fills `p` with the defaults of main.h:78-106. */
void dpe_params_default(DpePatchMatchParams* p);

/*
 * Inputs of one PatchMatch pass for one reference image, all HOST pointers, row-major.
 * Index 0 is the reference image, 1..num_images-1 the source images (DPE.cpp:743-761).
 */
typedef struct DpePassInput {
  int width, height;               /* pass resolution (after the caller's rescale) */
  int num_images;                  /* <= DPE_MAX_IMAGES */
  const float* const* images;      /* [num_images] -> f32 [H][W] grey levels (DPE.cpp:745-757) */
  const DpeCamera* cams;           /* [num_images], K already scale-adjusted (DPE.cpp:814-819) */
  const float* const* depths;      /* [num_images] -> f32 [H][W], NULL unless geom (DPE.cpp:826-843);
                                      entry 0 may be NULL (the ref depth is never sampled) */
  const uint8_t* edge;             /* [H][W] {0,255} edges_<scale>.dmb, or NULL (DPE.cpp:1032) */
  int low_width, low_height;       /* size of edge_low_res */
  const uint8_t* edge_low_res;     /* [lh][lw] edges_<max_scale>.dmb (DPE.cpp:1042), or NULL */
  const int32_t* label;            /* [H][W] labels_<scale>.dmb, or NULL (DPE.cpp:1049) */
  DpePatchMatchParams params;      /* params.num_images / depth_min / depth_max set by caller */
  uint64_t seed;                   /* Philox key (the reference seeds cuRAND from clock64()) */
  uint32_t pass_salt;              /* distinguishes passes that reuse a seed */
  const int32_t* image_ids;        /* [num_images] or NULL.  With ids, each image's device copy and its
                                      gather layouts stay resident in HBM keyed by (id, width, height)
                                      and later passes skip the upload (the caller promises that an
                                      id at a size always has the same pixels); NULL: upload every pass */
} DpePassInput;

/*
 * Per-pixel state, in/out, HOST pointers.
 *  planes:         float4 [H][W]; in: (world normal xyz, depth w) prior unless FIRST_INIT
 *                  (DPE.cpp:896-903); out: (world normal xyz, depth w) (DPE.cu:1940-1955).
 *  weak_info:      u8 [H][W] PixelState; in: weak.bin (ignored, all STRONG, when !use_APD,
 *                  DPE.cpp:873-881); out: DepthToWeak classification (DPE.cu:2593-2747).
 *  selected_views: u32 [H][W] view bit-mask, in/out (DPE.cpp:906-911).
 *  costs:          f32 [H][W] optional output (NULL to skip); not in the reference's readback.
 */
typedef struct DpePassState {
  float* planes;
  uint8_t* weak_info;
  uint32_t* selected_views;
  float* costs;
} DpePassState;

typedef struct DpeContext DpeContext;

/* Context = one HIP device + its workspaces.  One context per thread. */
DpeContext* dpe_create(int device);
void dpe_destroy(DpeContext* ctx);

/* Last error message of the calling thread ("" if none). */
const char* dpe_last_error(void);

/* Uploads inputs and the initial state (H2D), builds the device layouts. Synchronous.  Waits first
 * for the work of the previous dpe_pm_execute (on whatever stream it was enqueued), so stage(A);
 * execute(A, s); stage(B) never overwrites inputs pass A still reads. */
int dpe_pm_stage(DpeContext* ctx, const DpePassInput* in, const DpePassState* state);

/*
 * Runs the whole pass (DPE.cu:3150-3226) on device-resident data on `stream` (a hipStream_t,
 * NULL = the context's stream).  Every call starts from the staged initial state, so repeated
 * calls are idempotent.  Asynchronous w.r.t. the host; ordered after the previous execute (the stream
 * waits on its completion event), and dpe_pm_stage / dpe_pm_fetch / dpe_destroy wait for it.
 * Part of the pass runs on the context's second (aux) stream, forked from and joined back into
 * `stream` with events, so all work is complete when `stream` reaches the end of the call's
 * enqueued work (environment DPE_OVERLAP=0, timing or counting keep everything on `stream`).
 * The aux stream runs the setup chain: GenEdgeInform and its edge-ray line scans,
 * FindNearestStrongPoint's tables and search, the WEAK-pixel list, GenNeighbours (the scratch-free
 * kernel, its coordinate tables and the scratch kernel for its overflow pixels) and NeigbourUpdate.
 * Beside it `stream` runs
 * RandomInitialization (reads planes/sel/images, writes planes/costs/sel) and the iteration-0
 * colour-0 strong half-sweep, which waits for GenEdgeInform's event only (it reads the edge rays;
 * it must not read nearest, nb, weak_rel or radius, which the aux stream is still writing); every
 * later launch waits for the join.  tests/test_gpu_parity.py checks the forked and one-stream
 * schedules bit for bit, including weak, sel and costs.
 */
int dpe_pm_execute(DpeContext* ctx, void* stream);

/* D2H of the outputs (DPE.cu:3245-3247).  Synchronous. */
int dpe_pm_fetch(DpeContext* ctx, const DpePassState* state);

/* stage + execute + fetch. */
int dpe_pm_run(DpeContext* ctx, const DpePassInput* in, const DpePassState* state);

/* Drops every image kept by `image_ids` (frees their HBM). */
void dpe_image_cache_clear(DpeContext* ctx);

/* Device pointer of the working planes buffer (float4 [H][W]) for device-side consumers
 * (e.g. the depth all-gather of the multi-GPU schedule).  NULL before dpe_pm_stage. */
void* dpe_pm_device_planes(DpeContext* ctx);

/* Copies depth (planes.w) into a caller device buffer f32 [H][W] on `stream`. */
int dpe_pm_export_depth(DpeContext* ctx, float* dev_dst, void* stream);

/*
 * HBM-resident pipeline state: the reference writes each image's depths.dmb / normals.dmb / weak.bin /
 * selected_views.bin after a pass (main.cpp:439-446) and its next pass, or a neighbour's geometric
 * term, reads them back (DPE.cpp:826-911).  Here they stay on the device, keyed by image id.
 *
 * dpe_state_save:      after dpe_pm_execute, applies ProcessProblem's epilogue (main.cpp:423-437: depth
 *                      outside [params.depth_min, depth_max] -> 0 and UNKNOWN) on the device and keeps
 *                      (world normal, depth, weak, selected views) as image_id's state.
 * dpe_pm_stage_resident: dpe_pm_stage whose initial state (planes unless FIRST_INIT, weak when use_APD,
 *                      selected views unless FIRST_INIT) comes from prior_id's state, and whose source depths
 *                      (geom_consistency) come from the states of in->image_ids[1..]: each rescaled on the
 *                      device with RescaleMatToTargetSize's nearest rule (DPE.cpp:1146-1165), exactly as the
 *                      host path rescales them.  in->depths is ignored; in->image_ids is required for geom.
 * dpe_state_snapshot:  copies every state's depth into its snapshot and makes later resident stages read
 *                      source depths from the snapshots (the Jacobi schedule: every pass of a round sees the
 *                      previous round's depths).
 * dpe_state_fetch:     host copies of a state (any output pointer may be NULL); w, h receive its size.
 * dpe_state_export_depth / dpe_state_import_depth: the depth map of a state to / from a caller device
 *                      buffer f32 [h][w] on `stream` (the multi-rank all-gather; an imported id without a
 *                      pass of its own holds a depth map only).
 * dpe_state_clear:     frees every state.
 */
int dpe_state_save(DpeContext* ctx, int image_id);
int dpe_pm_stage_resident(DpeContext* ctx, const DpePassInput* in, int prior_id);
int dpe_state_snapshot(DpeContext* ctx);
int dpe_state_fetch(DpeContext* ctx, int image_id, int* w, int* h, float* depth, float* normal, uint8_t* weak,
                    uint32_t* selected_views);
int dpe_state_export_depth(DpeContext* ctx, int image_id, float* dev_dst, void* stream);
int dpe_state_import_depth(DpeContext* ctx, int image_id, int w, int h, const float* dev_src, void* stream);
void dpe_state_clear(DpeContext* ctx);
/* Context-owned device scratch of `count` floats (slot 0 or 1; grows, kept until dpe_destroy) and a
 * synchronous copy (kind 0 host->device, 1 device->host, 2 device->device) after all work of the
 * context: the exchange buffers of the multi-rank schedule without HIP in the caller. */
float* dpe_device_buffer(DpeContext* ctx, int slot, size_t count);
int dpe_device_copy(DpeContext* ctx, void* dst, const void* src, size_t bytes, int kind);
/* Blocks until every operation queued on the context (pass, state exports / imports) has finished,
 * e.g. before a caller's collective reads a buffer an export filled.  DPE_OK or an error code. */
int dpe_sync(DpeContext* ctx);

/*
 * EdgeSegment's data-parallel stages on the device (DPE.cpp:129-291 calls them through OpenCV; the
 * host restatement is host/edges.cpp, and these are bit-identical to it).  HOST buffers, synchronous,
 * on the context's stream (use one context per thread, or serialise the calls).
 *   dpe_resize_linear      cv::resize(INTER_LINEAR) of CV_32FC1             == dpe_host_resize_linear
 *   dpe_resize_u8          cv::resize(INTER_LINEAR) of CV_8UC1 (INTER_AREA fast path at exactly 1/2)
 *                                                                          == dpe_host_resize_u8
 *   dpe_canny              cv::Canny(L2gradient, aperture 3): Sobel, magnitude, non-maximum
 *                          suppression and the strong candidates on the device, the 8-connected
 *                          hysteresis walk on the host                      == dpe_host_canny
 *   dpe_roberts_threshold  Roberts (DPE.cpp:9-25) + cv::threshold(thr, 255, THRESH_BINARY)
 * Connect (DPE.cpp:27-127) and HoughLinesP are scan-order / RNG-order dependent and stay on the host.
 */
int dpe_resize_linear(DpeContext* ctx, const float* src, int w, int h, float* dst, int nw, int nh);
int dpe_resize_u8(DpeContext* ctx, const uint8_t* src, int w, int h, uint8_t* dst, int nw, int nh);
int dpe_canny(DpeContext* ctx, const uint8_t* src, int w, int h, double low, double high, uint8_t* dst);
int dpe_roberts_threshold(DpeContext* ctx, const uint8_t* src, int w, int h, int thr, uint8_t* dst);

/* Kernel classes of one pass, for timing and work accounting. */
enum {
  DPE_CLASS_SETUP = 0,        /* GenEdgeInform, FindNearestStrongPoint, GenNeighbours, NeigbourUpdate */
  DPE_CLASS_INIT = 1,         /* RandomInitialization */
  DPE_CLASS_STRONG = 2,       /* Black/RedPixelUpdateStrong */
  DPE_CLASS_RANSAC = 3,       /* RANSACToGetFitPlane */
  DPE_CLASS_WEAK = 4,         /* Black/RedPixelUpdateWeak */
  DPE_CLASS_FILTER = 5,       /* GetDepthandNormal + Black/RedPixelFilterStrong */
  DPE_CLASS_DEPTH_TO_WEAK = 6,/* DepthToWeak */
  DPE_CLASS_LOCAL_REFINE = 7, /* LocalRefine */
  DPE_NUM_CLASSES = 8
};

/* Enables hipEvent timing of every launch of the following dpe_pm_execute calls. */
void dpe_set_timing(DpeContext* ctx, int enable);
/* ms[0] = whole pass (first to last event), ms[1 + c] = summed kernel time of class c.
 * Returns the number of entries written (<= n, at most 1 + DPE_NUM_CLASSES). */
int dpe_pm_last_timings(DpeContext* ctx, float* ms, int n);

/* Enables algorithmic work counters (device atomics; a counting run is slower and is never the
 * timed run).  out[4*c + k] for class c: k=0 homography set-ups (NCC evaluations), k=1 bilinear
 * taps, k=2 geometric-consistency evaluations, k=3 launches.  Returns entries written. */
void dpe_set_counting(DpeContext* ctx, int enable);
int dpe_pm_last_counts(DpeContext* ctx, unsigned long long* out, int n);

/* Diagnostic knobs and statistics of the pass (not part of the reference's surface; tests).
 * DPE_OPT_GN_SLOTS: support-point slots per WEAK pixel of the scratch-free GenNeighbours
 *   (k_gen_neighbours_lds): 0 = by rotate_time (32 up to 2, else 64, enough for every pixel), 8 = a
 *   test setting that sends every pixel with more points through the overflow path (the scratch
 *   kernel).  Results are the same for every setting.
 * DPE_STAT_GN_DEFERRED: WEAK pixels the scratch-free GenNeighbours of the last execute handed to the
 *   scratch kernel (more points than slots, or a NaN in its sorts).  Synchronises with the pass.
 * DPE_STAT_TEX_CLASS: texel layouts of the staged images: 2 = every grey level an integer in
 *   [0, 255] (u8 / f16 texels), 1 = every grey level a multiple of 1/4 in [0, 255] (the exact 1/2
 *   and 1/4 downscales of the coarse pyramid levels: f16 texels), 0 = f32 texels.
 * dpe_set_option returns DPE_OK or DPE_ERR_ARG; dpe_pm_last_stat returns the value or -1. */
enum { DPE_OPT_GN_SLOTS = 1 };
enum { DPE_STAT_GN_DEFERRED = 1, DPE_STAT_TEX_CLASS = 2 };
int dpe_set_option(DpeContext* ctx, int option, int value);
long long dpe_pm_last_stat(DpeContext* ctx, int stat);

/*
 * RunFusion (DPE.cpp:1220-1370): the per-(pixel, source view) projection tests on the GPU.  The
 * order-dependent rest (the masks of already fused pixels, the angle test, the consistency weights,
 * colours) stays with the caller, in the reference's serial order (the host pipeline's fusion).
 */
typedef struct DpeFusionView {
  int width, height;
  DpeCamera cam;              /* ReadCamera, scaled to the map size (RescaleImageAndCamera, DPE.cpp:1123) */
  const float* depth;         /* f32 [H][W] final depth (depths.dmb; <= 0: no depth) */
  const float* normal;        /* f32 [H][W][3] final world normals (normals.dmb) */
} DpeFusionView;

/* Uploads every view's depth and normal map (H2D); they stay resident for dpe_fusion_candidates. */
int dpe_fusion_stage(DpeContext* ctx, const DpeFusionView* views, int n_views);

/* For reference view `ref` and its source views src[0..ns-1] (indices into the staged views),
 * pixel p (row-major) and source j (DPE.cpp:1303-1343 without the masks):
 *   idx[p*ns + j] = row-major source pixel int(y+.5)*W + int(x+.5) of the projection when it lies
 *                   inside the source view on a depth > 0 with reprojection error < 2 and relative
 *                   depth difference < 0.01; else -1;
 *   val[(p*ns + j)*3 + k] = (reprojection error, relative depth difference, n_ref . n_src).
 * HOST output buffers of W*H*ns int32 / W*H*ns*3 floats.  Synchronous. */
int dpe_fusion_candidates(DpeContext* ctx, int ref, const int* src, int ns, int32_t* idx, float* val);

/*
 * The two Tanks-and-Temples fusions, RunFusion_TAT_Intermediate (DPE.cpp:1372-1540) and
 * RunFusion_TAT_advanced (DPE.cpp:1542-1689), one whole image on the device (csrc/pass_fusion_tat.h):
 * these variants set only the fused pixel's own mask, so the pixels of an image are independent and
 * only the images are sequential.  The reference's per-view `diff` entries, never reset between
 * pixels, are reproduced as a last-hit carry over the raster.
 *
 * dpe_fusion_tat_begin:  after dpe_fusion_stage; uploads the colour image (u8 [H][W][3] BGR at the map
 *                  size) and the optional block mask (u8 [H][W]; `block` or an entry may be NULL) of every
 *                  staged view and zeroes the fusion masks.  Synchronous.
 * dpe_fusion_tat_image:  fuses reference view `ref` against src[0..ns-1] (indices of staged views, none
 *                  equal to `ref`, ns <= 31) in `mode` (DPE_FUSION_TAT_*).  Images must be fused in the
 *                  run's order: the masks of earlier calls are read.  dot_thresholds[k], k = 2..ns: the
 *                  smallest dot product in [-1, 1] that passes the angle test at k (Intermediate;
 *                  dpe_host_fusion_tat_thresholds builds it; ignored for Advanced).  *n receives the
 *                  number of points, in raster order; more than `cap` is DPE_ERR_ARG.  The kernels have
 *                  finished on return, but the copy of the points into `out` runs on beside the next
 *                  call's kernels: `out` is complete, and may be released, when the next
 *                  dpe_fusion_tat_image, dpe_fusion_tat_wait or dpe_destroy returns.
 * dpe_fusion_tat_mask:   host copy of a view's fusion mask u8 [H][W] (tests).  Synchronous.
 */
enum { DPE_FUSION_ETH3D = 0, DPE_FUSION_TAT_INTERMEDIATE = 1, DPE_FUSION_TAT_ADVANCED = 2 };
typedef struct DpeFusedPoint { float x, y, z, b, g, r; } DpeFusedPoint;   /* PointList: world point, float BGR */
int dpe_fusion_tat_begin(DpeContext* ctx, const uint8_t* const* bgr, const uint8_t* const* block);
int dpe_fusion_tat_image(DpeContext* ctx, int mode, int ref, const int* src, int ns, const float* dot_thresholds,
                         DpeFusedPoint* out, size_t cap, size_t* n);
int dpe_fusion_tat_wait(DpeContext* ctx);
int dpe_fusion_tat_mask(DpeContext* ctx, int view, uint8_t* mask);

/*
 * Consistency maps of one reference view (csrc/pass_consistency.h), after dpe_fusion_stage: for
 * reference view `ref`, its source views src[0..ns-1] (indices into the staged views, none equal to
 * `ref`, ns <= 255) and pixel p (row-major),
 *   count[p]          = the number of j for which RunFusion's view loop (DPE.cpp:1312-1343) reaches
 *                       num_consistent++ with its masks[...] tests and the blocks test removed: reference
 *                       depth > 0, projection inside view src[j] (x + 0.5, y + 0.5 in (-1, size), tested on
 *                       the float) on a depth > 0, reprojection error < 2.0f (squares, sum and root in
 *                       double, rounded once), relative depth difference < 0.01f, and the angle test
 *                       `!(dot >= -1 && dot <= 1) || dot >= dot_threshold`, which is
 *                       GetAngle(n_ref, n_src) < 0.174533f when dot_threshold comes from
 *                       dpe_host_consistency_dot_threshold (dpe_host.h);
 *   depth_filtered[p] = count[p] >= min_views ? depth_ref[p] : 0.0f.
 * RunFusion's dynamic_consistency weight is not part of this.  Bit-identical to dpe_host_consistency.
 * HOST output buffers of W*H uint8 / floats of the reference view; either may be NULL (no copy).
 * Synchronous.  ns = 0 gives all zeros.  DPE_ERR_ARG: ns < 0 or > 255, min_views outside 1..255, an
 * index outside the staged views, `ref` among `src`; DPE_ERR_STATE: nothing staged.
 * dpe_consistency_launches: kernels of this section launched by the process so far (a run without the
 * option launches none).
 */
int dpe_fusion_consistency(DpeContext* ctx, int ref, const int* src, int ns, float dot_threshold, int min_views,
                           uint8_t* count, float* depth_filtered);
long long dpe_consistency_launches(void);

/* Page-locks (pins) / releases a caller's host buffer so that device -> host copies into it run at
 * full PCIe rate (hipHostRegister; the host fusion pins its candidate buffers).  Nonzero when the
 * runtime refuses (no device, limits): the buffer then stays pageable and every call still works. */
int dpe_host_pin(void* ptr, size_t bytes);
int dpe_host_unpin(void* ptr);

/*
 * The viz medium results (ShowDepthMap / ShowNormalMap / ShowWeakImage, DPE.cpp:384-502, and the
 * data-parallel half of cv::imwrite's JPEG encode) from an HBM-resident state, after dpe_state_save.
 * The pictures are bit-identical to dpe_host_viz_render and the blocks to dpe_host_jpeg_blocks
 * (include/dpe_host.h, which also documents the block layout); no float image crosses PCIe.
 *
 * dpe_state_render:  image_id's state as 8-bit BGR [h][w][3] into a HOST buffer.  Synchronous.
 * dpe_state_render_jpeg_blocks: renders, runs the JPEG front half (BGR -> YCbCr 4:2:0, edge
 *                    replication, forward DCT, quantisation at `quality`) and copies the
 *                    ceil(w/16) * ceil(h/16) * 6 * 64 int16 values into host_blocks (`cap` in int16;
 *                    pin it with dpe_host_pin for an asynchronous copy).  Enqueued on `stream`
 *                    (NULL = the context's); complete at dpe_sync, or when dpe_state_render_wait
 *                    (ctx, host_blocks), which any host thread may call, returns.
 * Both are ordered by the stream only: a later pass of the same image runs after them.
 * DPE_ERR_STATE for an unknown id or a depth-only (imported) state, DPE_ERR_ARG for a bad kind or a
 * cap that is too small.
 *
 * Diagnostic entries (tests) through the same kernels: dpe_viz_render_arrays renders caller HOST
 * arrays (depth f32 [h][w], normal f32 [h][w][3], weak u8 [h][w]; those the kind does not read may
 * be NULL), dpe_jpeg_blocks_device runs the front half on a caller HOST BGR image; both synchronous.
 * dpe_viz_launches: kernels of this section launched by the process so far (a run with viz = false
 * launches none).
 */
enum { DPE_VIZ_DEPTH = 0, DPE_VIZ_NORMAL = 1, DPE_VIZ_WEAK = 2 };
int dpe_state_render(DpeContext* ctx, int image_id, int kind, float depth_min, float depth_max, uint8_t* host_bgr);
int dpe_state_render_jpeg_blocks(DpeContext* ctx, int image_id, int kind, float depth_min, float depth_max, int quality,
                                 int16_t* host_blocks, size_t cap, void* stream);
int dpe_state_render_wait(DpeContext* ctx, const int16_t* host_blocks);
int dpe_viz_render_arrays(DpeContext* ctx, int kind, int w, int h, const float* depth, const float* normal,
                          const uint8_t* weak, float depth_min, float depth_max, uint8_t* host_bgr);
int dpe_jpeg_blocks_device(DpeContext* ctx, const uint8_t* host_bgr, int w, int h, int quality, int16_t* host_blocks,
                           size_t cap);
long long dpe_viz_launches(void);

/*
 * ExportDepthImagePointCloud (DPE.cpp:1691-1724; its call is the commented block at main.cpp:456-466):
 * one image's depth map back-projected into coloured points, from the HBM-resident state after
 * dpe_state_save (csrc/pass_points.h).  Bit-identical to dpe_host_depth_point_cloud (dpe_host.h).
 *
 * A pixel is skipped when `depth < depth_min || depth > depth_max || isnan(depth)` (both ends kept,
 * NaN tested on the bit pattern).  `mode` DPE_POINTS_ALL: the depth as it is; DPE_POINTS_STRONG
 * (main.cpp:464): a pixel whose state is not DPE_STRONG has its depth replaced by 0 BEFORE the test
 * (with depth_min <= 0 it is emitted at depth 0).  The points come in the reference's order: columns
 * outside, rows inside.  A point is Get3DPointonWorld(column, row, depth, cam) and the colour image's
 * (B, G, R) at that pixel as floats.
 *
 * dpe_state_point_cloud:  image_id's state; `cam` and `host_bgr` (u8 [h][w][3]) are already at the map
 *                    size (RescaleImageAndCamera).  Uploads the colours, runs the kernels on `stream`
 *                    (NULL = the context's) and waits for them: *n is the number of points on return
 *                    (more than `cap` is DPE_ERR_ARG and copies nothing).  Only the n points are then
 *                    copied into the HOST buffer `out` (pin it with dpe_host_pin for an asynchronous
 *                    copy); the copy is complete at dpe_sync, or when dpe_state_point_cloud_wait(ctx, out),
 *                    which any host thread may call, returns.  DPE_ERR_STATE for an unknown id, and in
 *                    DPE_POINTS_STRONG for a depth-only (imported) state; DPE_ERR_ARG for a bad mode.
 * dpe_point_cloud_arrays: the diagnostic twin (tests) over caller HOST arrays (depth f32 [h][w], weak u8
 *                    [h][w], NULL allowed in DPE_POINTS_ALL, bgr u8 [h][w][3]) through the same kernels.
 *                    Synchronous.
 * dpe_points_launches: kernels of this section launched by the process so far (a run without point
 *                    clouds launches none).
 */
enum { DPE_POINTS_ALL = 1, DPE_POINTS_STRONG = 2 };
int dpe_state_point_cloud(DpeContext* ctx, int image_id, int mode, const DpeCamera* cam, const uint8_t* host_bgr,
                          float depth_min, float depth_max, DpeFusedPoint* out, size_t cap, size_t* n, void* stream);
int dpe_state_point_cloud_wait(DpeContext* ctx, const DpeFusedPoint* out);
int dpe_point_cloud_arrays(DpeContext* ctx, int mode, int w, int h, const float* depth, const uint8_t* weak,
                           const DpeCamera* cam, const uint8_t* bgr, float depth_min, float depth_max, DpeFusedPoint* out,
                           size_t cap, size_t* n);
long long dpe_points_launches(void);

/*
 * Cloud evaluation: the exact truncated nearest-neighbour distance between two point clouds, the measurement
 * behind precision / recall / F-score of a PLY (dpe_host_cloud_eval, dpe_host.h).  No counterpart in the
 * reference, which publishes no accuracy figure.
 *
 * Clouds are packed f32 [k][3] HOST arrays; radius R is a finite float > 0; n, m <= 2^31 - 1; anything else
 * is DPE_ERR_ARG.  All in float, every operation rounded, no contraction:
 *   d2(q, t):  dx = q.x - t.x; dy = q.y - t.y; dz = q.z - t.z;  s = dx*dx; s = s + dy*dy; s = s + dz*dz
 *   out[i] = min(R2, min_j d2(Q[i], T[j])),  R2 = R*R            (the SQUARED distance, f32 [n])
 * A target point with a non-finite coordinate is skipped; a query point with one gets R2; m = 0 gives all R2.
 * The result is a minimum over a set: the bits of a serial loop over the target, whatever the schedule
 * (dpe_host_cloud_nn gives the same bits on host threads).  A hashed uniform grid of edge R * (1 + 2^-10)
 * over the target and a 27-cell query; csrc/cloud_dist.h states why that covers every t with d2 < R2.
 * A target whose extent over that edge reaches 2^30 cells on an axis is DPE_ERR_ARG ("radius too small for
 * the cloud's extent").
 *   dpe_cloud_nn            one direction.  Synchronous: d2_out is complete when it returns.
 *   dpe_cloud_nn_pair       both directions, each cloud staged once: a_to_b f32 [n], b_to_a f32 [m].
 *   dpe_cloud_launches      kernels of this section launched by the process so far (a run that never asks
 *                           for an evaluation launches none).
 *   dpe_cloud_last_timings  with dpe_set_timing on: device milliseconds of the last call's parts, [0] stage
 *                           (upload), [1] grid build, [2] query, [3] download, summed over the directions;
 *                           returns the number of entries written (<= n, at most 4; 0 when none was timed).
 * The buffers belong to the context, grow on demand, are freed by dpe_destroy and count in
 * dpe_live_device_bytes.
 */
int dpe_cloud_nn(DpeContext* ctx, const float* query, size_t n, const float* target, size_t m, float radius,
                 float* d2_out);
int dpe_cloud_nn_pair(DpeContext* ctx, const float* a, size_t n, const float* b, size_t m, float radius, float* a_to_b,
                      float* b_to_a);
long long dpe_cloud_launches(void);
int dpe_cloud_last_timings(DpeContext* ctx, float* ms, int n);

/*
 * Voxel down-sampling: one record per non-empty voxel of a cloud, what the ETH3D and Tanks-and-Temples tools
 * do to both clouds before they score, and a way to thin a fused cloud.  No counterpart in the reference.
 *
 * Inputs (HOST arrays): n points, packed f32 [n][3], n <= 2^31 - 1; optionally n colours, u8 [n][3] (three
 * channels in the caller's order, each treated alike); a voxel edge v, a finite float > 0.  Anything else is
 * DPE_ERR_ARG ("bad argument").
 * Output, k records: xyz f32 [k][3]; rgb u8 [k][3] (only when colours were given); first i32 [k]; count i32 [k].
 *
 * Cell of a point.  A point with a non-finite coordinate belongs to no voxel.  o[a] = the per-axis minimum of
 * the finite points as a double, h = (double)v, u = ((double)x - o) / h, c = floor(u) (dpe_cloud_nn's cell
 * arithmetic).  An extent (max - min) / h of 2^30 cells or more on an axis, decided on the double, is
 * DPE_ERR_ARG ("voxel too small for the cloud's extent").
 * Position.  The centroid is taken on a lattice of 2^32 steps per voxel edge, so that it is an exact integer
 * sum and depends on no order: per point and axis f = u - c (exact, in [0, 1)) and q = (uint64)(f * 2^32),
 * truncated; per voxel and axis S = sum of q in uint64 (below 2^63 for any n); the coordinate is
 *   (float)(o + ((double)c + ((double)S / (double)count) * 2^-32) * h)
 * every operation a rounded double operation in exactly this order, without contraction.  The lattice costs less
 * than h * 2^-32 per coordinate against the real-number centroid.  A voxel that holds ONE point may return that
 * point moved by one float ulp: the record is the lattice expression above, not a copy of the input.
 * Colour.  Per channel (2 * sum + count) / (2 * count) in integers, the mean rounded half up; the sums are
 * 64 bits wide, exact for any n.
 * first = the lowest original index among the voxel's points, count = their number.
 * Order.  Ascending `first`: the order in which a serial loop over the points meets the voxels.
 * Everything in a record is a sum, a minimum or a count over a set, so the result is the serial loop's to the
 * bit whatever the schedule (dpe_host_cloud_voxel, dpe_host.h, is that loop).
 *
 *   dpe_cloud_voxel  writes at most `cap` records and their number into *k.  With more voxels than `cap` it
 *                    writes no record, stores the number of voxels in *k and returns DPE_ERR_ARG (cap = n
 *                    always fits).  n = 0 or no finite point: *k = 0 and no kernel beyond the staging of the
 *                    cloud.  Concurrency as dpe_cloud_nn: waits until the context is quiet, runs on its stream,
 *                    synchronous.  An open-addressing table over the cells (csrc/pass_voxel.h); its buffers
 *                    belong to the context like dpe_cloud_nn's, every launch counts in dpe_cloud_launches, and
 *                    dpe_cloud_last_timings then reports [0] stage, [1] cells + insert, [2] emit, [3] download.
 */
int dpe_cloud_voxel(DpeContext* ctx, const float* xyz, size_t n, const uint8_t* rgb_or_null, float voxel, float* out_xyz,
                    uint8_t* out_rgb, int32_t* out_first, int32_t* out_count, size_t cap, size_t* k);

/*
 * Rigid registration of two clouds: the nearest neighbour WITH its index, and one step of point-to-point ICP
 * reduced to 16 sums and a count (the solve and the loop are the host's: dpe_host_cloud_register, dpe_host.h).
 * No counterpart in the reference.  Clouds, radius and refusals are dpe_cloud_nn's.
 *
 * Nearest neighbour with index.  idx[i] = the j that minimises the pair (d2(Q[i], T[j]), j) lexicographically
 * over the finite T[j] with d2 < R2; d2, R2 = R*R and the strict < are dpe_cloud_nn's, and d2_out[i] is what
 * dpe_cloud_nn returns.  idx[i] = -1 when nothing is within R, when the query is non-finite and when the target
 * is empty.  A lexicographic minimum over a set does not depend on the order in which the candidates are met:
 * the result is a serial loop's to the bit (dpe_host_cloud_nn_index is that loop over the same grid).
 *
 * One ICP step.  Source P (n points), target G (m points), radius R, transform T: 12 doubles, row-major 3 x 4,
 * [R | t].  Per source index i with a finite P[i]:
 *   x' = (float)(((T[0]*x + T[1]*y) + T[2]*z) + T[3]),  y', z' from rows 1 and 2
 * in double, every operation rounded, in this order, no contraction.  (x', y', z') is matched against G by the
 * rule above; a non-finite P[i] or a non-finite image has no match.  A source without a match contributes +0.0
 * to every sum.  A matched source (to G[j] at squared distance d2) contributes the 16 terms
 *   (double)d2,  a[r] = (double)P[i][r] - o_s[r],  b[c] = (double)G[j][c] - o_t[c],  a[r] * b[c]   (r, c in 0..2)
 * where o_s and o_t are the per-axis minima of each cloud's finite points as doubles (the centring keeps a cloud
 * at an offset of +-1000 from cancelling in sum(ab) - sum(a) sum(b) / N) and the products are rounded doubles.
 * Each of the 16 sums is taken by PAIRWISE SUMMATION IN INDEX ORDER: level 0 is the n terms, level l + 1 has
 * s[k] = s_l[2k] + s_l[2k + 1] with +0.0 for a missing right operand, until one value is left.  Addition is
 * commutative, so an xor butterfly gives these bits in every lane, and 256 consecutive leaves are a complete
 * subtree, so blocks of 256 and further levels over the block results are the same tree.  The terms are indexed
 * by SOURCE index, so a fixed tree over that index costs nothing to fix and plain doubles do (the voxel
 * centroid sums per cell in an order only a sort could fix, which is why it went to an integer lattice).  The
 * matched count is an integer.  dpe_host_cloud_icp_step (dpe_host.h) takes the tree literally: the same bits.
 *
 *   dpe_cloud_nn_index   one direction with indices: d2_out f32 [n], idx_out i32 [n].  Synchronous.
 *   dpe_cloud_icp_stage  uploads both clouds, takes their bounds and builds the target's grid for `radius` once;
 *                        clouds and grid stay resident until the next cloud call of the context.  Call it again
 *                        for the next radius of a schedule.
 *   dpe_cloud_icp_step   one step over what is staged: T goes up (96 bytes), DpeIcpSums comes down.  Without a
 *                        staged pair DPE_ERR_STATE.  dpe_cloud_last_timings then reports [0] apply + build of the
 *                        transformed source, [1] match, [2] sums, [3] download.
 * Concurrency, error strings, dpe_cloud_launches and the buffers are dpe_cloud_nn's.
 */
typedef struct DpeIcpSums {
  long long matched;
  double d2, a[3], b[3], ab[9];         /* ab[3 * r + c] = sum of a[r] * b[c] */
} DpeIcpSums;
int dpe_cloud_nn_index(DpeContext* ctx, const float* query, size_t n, const float* target, size_t m, float radius,
                       float* d2_out, int32_t* idx_out);
int dpe_cloud_icp_stage(DpeContext* ctx, const float* src, size_t n, const float* tgt, size_t m, float radius);
int dpe_cloud_icp_step(DpeContext* ctx, const double* T, DpeIcpSums* out);

/*
 * Depth-map evaluation: a ground-truth scan rendered into one camera with a z-buffer, and an estimated depth map
 * compared with such a map pixel by pixel: how the ETH3D and DTU tools get per-view ground truth.  No
 * counterpart in the reference.  All in float unless a double is written, every operation rounded, IEEE
 * division, no contraction (csrc/depth_eval.h holds the arithmetic once, for the kernels and the host loops).
 *
 * Render.  A cloud f32 [n][3] (HOST array, n <= 2^31 - 1), a DpeCamera already at the map's size (width,
 * height >= 1), a splat half-width s in 0..8; anything else is DPE_ERR_ARG.  Output f32 [height][width].
 * Per point with three finite coordinates (decided on the bit patterns):
 *   (px, py, z) = ProjectCamera in the reference's order (DPE.cpp:1196-1206), the expression of the fusion
 *   kept iff 0 < bits(z) < 0x7F800000 as an integer: positive and finite, a NaN excluded by its bits
 *   fx = px + 0.5f, fy = py + 0.5f; kept iff fx > -1 && fx < width && fy > -1 && fy < height on the floats
 *   (the fusion's rule); cx = (int)fx, cy = (int)fy, truncated
 *   the point covers the pixels (cx + dx, cy + dy), |dx|, |dy| <= s, that lie inside the image
 * out[p] = the minimum z over the points that cover p, 0.0f where none does.  A minimum over a set: the bits of
 * a serial loop whatever the schedule (on the device an integer atomic minimum on the bit pattern, since
 * positive finite floats order as their bits).  NO OCCLUSION TEST beyond the z-buffer is made: a sparse scan
 * lets far surfaces show between near points, and s trades that against dilated foreground edges.
 *
 * Score.  est and gt f32 [h][w] (w, h >= 1), 1 to 16 thresholds tau[k], each finite and >= 0, mode
 * DPE_DEPTH_TAU_ABS or DPE_DEPTH_TAU_REL; anything else is DPE_ERR_ARG.  Per pixel in index order:
 *   gt_ok, est_ok = the positive-finite bit test above; both = gt_ok && est_ok
 *   e = fabsf(est - gt); rel = e / gt
 *   hit[k] = both && (mode == ABS ? e < tau[k] : e < tau[k] * gt)          (strict, as in dpe_cloud_nn)
 * n_px = w * h, n_gt, n_est, n_both and within[k] count the pixels; sum_abs = sum of (double)e, sum_rel = sum of
 * (double)rel, sum_sq = sum of (double)e * (double)e, each over the `both` pixels and each by PAIRWISE SUMMATION
 * IN PIXEL-INDEX ORDER, the tree of dpe_cloud_icp_step above: s[k] = s[2k] + s[2k + 1], +0.0 for a missing
 * operand and for a pixel that is not `both` (so an image without a `both` pixel sums to +0.0).  The error map,
 * when asked for: e where both, -1.0f where gt_ok only, -2.0f otherwise.  Everything derived (accuracy,
 * completeness, means, RMSE) is the host's, in double: dpe_host_depth_stats (dpe_host.h).
 * dpe_host_cloud_render and dpe_host_depth_score (dpe_host.h) are the serial loops: the same bits.
 *
 *   dpe_cloud_render_stage  uploads the cloud once; it stays resident until the next cloud call of the context
 *                           (dpe_cloud_nn, _nn_pair, _nn_index, _voxel, _icp_stage), which ends the staging, as
 *                           this call ends a staged ICP pair.
 *   dpe_cloud_render_view   one view of the staged cloud (clear, one thread per point, a last pass that turns
 *                           empty pixels into 0.0f); the map stays resident for dpe_depth_score, and comes down
 *                           into depth_out when that is not NULL.  Without a staged cloud DPE_ERR_STATE.
 *   dpe_depth_score         gt == NULL: against the last rendered map, whose size must be w x h (else
 *                           DPE_ERR_ARG; DPE_ERR_STATE when no map was rendered); otherwise against the caller's
 *                           host array.  Blocks of 256 consecutive pixels, the butterfly of the ICP step, counts
 *                           by ballot; no float atomics.
 * Concurrency, error strings and the buffers are dpe_cloud_nn's; every launch counts in dpe_cloud_launches, and
 * dpe_cloud_last_timings then reports [0] stage (upload), [1] render, [2] score, [3] download of the last of
 * these calls (the parts it does not have are 0).  A refused call leaves the context and what is resident as
 * they were.
 */
#define DPE_DEPTH_MAX_TAU 16
#define DPE_DEPTH_MAX_SPLAT 8
#define DPE_DEPTH_TAU_ABS 0
#define DPE_DEPTH_TAU_REL 1
typedef struct DpeDepthScore {
  long long n_px, n_gt, n_est, n_both, within[DPE_DEPTH_MAX_TAU];
  double sum_abs, sum_rel, sum_sq;
} DpeDepthScore;
int dpe_cloud_render_stage(DpeContext* ctx, const float* xyz, size_t n);
int dpe_cloud_render_view(DpeContext* ctx, const DpeCamera* cam, int splat, float* depth_out_or_null);
int dpe_depth_score(DpeContext* ctx, const float* est, const float* gt_or_null, int w, int h, const float* tau, int n_tau,
                    int mode, DpeDepthScore* out, float* err_or_null);

/*
 * Normal-map evaluation: a normal for every point of a scan by PCA over its radius neighbourhood, the winning
 * point's normal rendered into a view beside the z-buffer depth, and an estimated normal map scored against such a
 * map pixel by pixel.  No counterpart in the reference.  csrc/normal_eval.h holds the arithmetic once, for the
 * kernels (csrc/pass_normals.h) and the host loops (host/normal_eval.cpp, dpe_host.h); every reduction is an integer
 * sum, a lexicographic minimum or the pairwise tree above, so the device gives the host loop's bits whatever the
 * schedule.  IEEE division and square root, no contraction.
 *
 * Point normals.  The cloud, R and the refusals are dpe_cloud_nn's; min_nb must be in 3..2^31-1 (DPE_ERR_ARG).
 *   N(i) = { j : P[j] finite, d2(P[i], P[j]) < R2 }   dpe_cloud_nn's d2, R2 = R*R and strict <; a finite point is
 *                                                    its own neighbour
 *   per neighbour and axis: dx = P[i].x - P[j].x in float (the term d2 forms), k = (int64)((double)dx * S) truncated
 *   toward zero, S = 32768.0 / (double)R, one rounded division.  |k| <= 2^15 + 1, so the largest sum of products
 *   stays below 2^62 for any n: that is why the lattice is 2^15 steps per radius and not finer.
 *   sums[10] (int64): the count; sum k_x, k_y, k_z; sum k_x k_x, k_x k_y, k_x k_z, k_y k_y, k_y k_z, k_z k_z.
 *   Integers: the serial loop's to the bit under any order (the voxel lattice's argument; a float covariance would
 *   depend on the slot order inside a bucket).
 *   C_ab = (double)m_ab - ((double)s_a * (double)s_b) / (double)cnt, rounded double operations in this order.
 *   The eigenvector of the smallest eigenvalue by cyclic Jacobi in double: pairs (0,1), (0,2), (1,2), always 8
 *   sweeps, a rotation skipped when its off-diagonal entry is 0; per rotation theta = (a_qq - a_pp) / (2 a_pq),
 *   t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c, a_pp -= t a_pq,
 *   a_qq += t a_pq, a_pq = 0, (a_rp, a_rq) = (c a_rp - s a_rq, s a_rp + c a_rq) and V's columns p, q likewise
 *   (csrc/normal_eval.h, normal_rotate, is the text).  Ties between eigenvalues go to the lowest index.  The vector
 *   is divided by its length in double, its sign chosen so that the component of largest magnitude is positive (a
 *   tie to the lowest axis), and rounded to float once.
 *   Valid iff cnt >= min_nb and the middle eigenvalue > 0 (not collinear, not one repeated point); otherwise the
 *   normal is (0, 0, 0), "no normal" everywhere below.  A non-finite point gets count 0, sums 0 and no normal.
 *
 * Render with normals.  Point, pixel and splat rules are dpe_cloud_render_view's.  The winner of a pixel is the
 * lexicographic minimum of (bits(z), point index) over the points that cover it; the depth map has
 * dpe_cloud_render_view's bits.  The normal map is f32 [h][w][3] in the WORLD frame (the frame of normal.npy).  A
 * pixel takes its winner's normal; if that is "no normal" (three zeros) or no point covers it, the pixel has none:
 * the winner decides, a farther point is never consulted.  Orientation towards the camera: p_cam = ProjectCamera's
 * (tx, ty, tz) of the winner, n_cam = R n row by row (TransformNormal2RefCam's order), s = (n_cam.x * p_cam.x +
 * n_cam.y * p_cam.y) + n_cam.z * p_cam.z in float; the world normal is negated iff s > 0.
 *
 * Score.  est and gt f32 [h][w][3]; 1 to 16 thresholds given as COSINES, each finite and in [-1, 1]; anything else
 * is DPE_ERR_ARG.  Per pixel in index order, in float:
 *   ee = (ex*ex + ey*ey) + ez*ez, gg likewise; est_ok = three finite components (by their bits) and 0 < bits(ee) <
 *   0x7F800000; gt_ok likewise; both = est_ok && gt_ok && the same test of ee * gg
 *   c = ((ex*gx + ey*gy) + ez*gz) / sqrtf(ee * gg), clamped to [-1, 1];  hit[k] = both && c > cos_tau[k]  (strict)
 *   bin = #{ b in 1..179 : c < E[b] },  E[b] = (float)cos((double)b * pi / 180): one host function fills E, for both
 *   paths; the device is handed the table and computes no cosine
 * n_px, n_gt, n_est, n_both, within[k], hist[bin] count the pixels (hist over the `both` pixels: its sum is n_both);
 * sum_dist = sum of 1.0 - (double)c and sum_dist_sq = sum of its square, each by PAIRWISE SUMMATION IN PIXEL-INDEX
 * ORDER (the tree of dpe_cloud_icp_step), a pixel that is not `both` adding +0.0.  The error map, when asked for: c
 * where both, -2.0f where only the ground truth has a normal, -3.0f otherwise.  Everything derived is the host's:
 * dpe_host_normal_stats (dpe_host.h).
 *
 *   dpe_cloud_normals              one grid of edge R over the cloud (target and query at once), one thread per
 *                                  point walking its 27 cells, a cell skipped when an earlier cell of the 27 gave
 *                                  its bucket already (so no point is counted twice), the solve in the same
 *                                  thread.  normal_out f32 [n][3], count_out i32 [n] (the count, at most n),
 *                                  sums_out i64 [n][10] or NULL.  Synchronous; ends any staging.
 *                                  dpe_cloud_last_timings: [0] stage, [1] build, [2] normals, [3] download.
 *   dpe_cloud_render_stage_normals dpe_cloud_render_stage plus the per-point normals f32 [n][3] (from
 *                                  dpe_cloud_normals or anywhere else); starts and ends as that staging does.
 *   dpe_cloud_render_view_normals  one view of a staging WITH normals (otherwise DPE_ERR_STATE, "no staged
 *                                  normals"); both outputs may be NULL.  The depth map becomes the resident map of
 *                                  dpe_depth_score, the normal map the resident map of dpe_normal_score.
 *                                  dpe_cloud_render_view on a staging with normals works as before.
 *   dpe_normal_score               gt == NULL: against the last rendered normal map (dpe_depth_score's rules).
 * Concurrency, error strings, buffers, dpe_cloud_launches and the timings' slots are dpe_cloud_render_view's.
 * Left out: point-to-plane ICP and normals in voxel records (which this unblocks), reading or writing a PLY with
 * normals, curvature or planarity output.
 */
#define DPE_NORMAL_MAX_TAU 16
#define DPE_NORMAL_BINS 180
typedef struct DpeNormalScore {
  long long n_px, n_gt, n_est, n_both, within[DPE_NORMAL_MAX_TAU], hist[DPE_NORMAL_BINS];
  double sum_dist, sum_dist_sq;
} DpeNormalScore;
int dpe_cloud_normals(DpeContext* ctx, const float* xyz, size_t n, float radius, int min_nb, float* normal_out,
                      int32_t* count_out, long long* sums_out_or_null);
int dpe_cloud_render_stage_normals(DpeContext* ctx, const float* xyz, const float* normals, size_t n);
int dpe_cloud_render_view_normals(DpeContext* ctx, const DpeCamera* cam, int splat, float* depth_out_or_null,
                                  float* normal_out_or_null);
int dpe_normal_score(DpeContext* ctx, const float* est, const float* gt_or_null, int w, int h, const float* cos_tau,
                     int n_tau, DpeNormalScore* out, float* err_or_null);

/* Device bytes held at the moment by every context of the process (their buffers, resident states and
 * cached images; tests: a destroyed context gives back all it allocated). */
long long dpe_live_device_bytes(void);

#ifdef __cplusplus
}
#endif
#endif /* DPE_MVS_H_ */
