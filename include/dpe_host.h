/*
 * dpe_host.h — C-ABI of the host pipeline (libdpe_host.so): the reference's RunDPEPipeline
 * (main.cpp:474-600) and the helpers it is built from, around the PatchMatch pass of dpe_mvs.h.
 *
 *   reference                                    replaced by
 *   -------------------------------------------  ------------------------------------------
 *   int RunDPEPipeline(path, gpu, bool x7)       dpe_run_pipeline(dense_folder, options)
 *     main.h:120, main.cpp:474
 *   ProcessProblem / DPE::InuputInitialization   (internal: one pass of one reference image)
 *     main.cpp:411-446, DPE.cpp:733-914
 *   cv::imread(IMREAD_GRAYSCALE)                 dpe_host_read_gray (JPEG islow luma / PGM)
 *   cv::resize(INTER_LINEAR)  DPE.cpp:808        dpe_host_resize_linear
 *   RescaleMatToTargetSize    DPE.cpp:1146       dpe_host_rescale_nearest
 *   EdgeSegment               DPE.cpp:129-291    dpe_host_edge_segment (GetProblemEdges, main.cpp:331,
 *                                                runs inside dpe_run_pipeline for missing maps)
 *   cv::Canny(L2, aperture 3) DPE.cpp:226        dpe_host_canny
 *   cv::resize INTER_LINEAR 8U DPE.cpp:145,230   dpe_host_resize_u8
 *   Connect                   DPE.cpp:27-127     dpe_host_connect
 *   RunFusion / ExportPointCloud DPE.cpp:1220,532 inside dpe_run_pipeline (fusion = true): projection
 *                                                tests on the GPU (dpe_fusion_candidates), serial rest
 *   RunFusion_TAT_Intermediate DPE.cpp:1372      inside dpe_run_pipeline, fusion_mode = DPE_FUSION_TAT_*: one
 *   RunFusion_TAT_advanced    DPE.cpp:1542       image at a time on the GPU (dpe_fusion_tat_image)
 *   cv::imread(IMREAD_COLOR)  DPE.cpp:1253       dpe_host_read_bgr
 *   cv::HoughLinesP           DPE.cpp:186        dpe_host_hough_lines_p
 *   ShowDepthMap              DPE.cpp:384-448    dpe_host_viz_render(DPE_VIZ_DEPTH)  (viz = true: on the
 *   ShowNormalMap             DPE.cpp:450-473    dpe_host_viz_render(DPE_VIZ_NORMAL)  GPU from the resident
 *   ShowWeakImage             DPE.cpp:475-502    dpe_host_viz_render(DPE_VIZ_WEAK)    state, dpe_state_render*)
 *   cv::imwrite(".jpg")       DPE.cpp:446, main.cpp:363  dpe_host_write_jpeg (libjpeg's defaults: quality 95,
 *                                                baseline, 4:2:0 / grey, Annex K Huffman tables)
 *   ExportDepthImagePointCloud DPE.cpp:1691      dpe_host_depth_point_cloud (point_cloud = 1 / 2: on the GPU
 *     (call commented out, main.cpp:456-466)     from the resident state, dpe_state_point_cloud)
 *   RescaleImageAndCamera     DPE.cpp:1123       dpe_host_rescale_image_and_camera
 *   (RunFusion's view loop without its masks,    dpe_host_consistency (consistency = min_views: per-image
 *     DPE.cpp:1312-1343; no such output there)   consistency.npy / depth_filtered.npy, on the GPU by
 *                                                dpe_fusion_consistency)
 *
 * Additions for the one-process-per-GPU deployment: a pass runner hook (default: the HIP library
 * on `gpu_index`) and an all-gather hook for the depth maps (RCCL in the CLI, torch.distributed
 * from Python).  Plain C types only.
 */
#ifndef DPE_HOST_H_
#define DPE_HOST_H_

#include <stddef.h>
#include <stdint.h>
#ifndef __cplusplus
#include <stdbool.h>
#endif

#include "dpe_mvs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Runs one PatchMatch pass: same contract as dpe_pm_run (stage + execute + fetch). */
typedef int (*dpe_pass_runner_fn)(void* user, const DpePassInput* in, const DpePassState* state);
/* All-gather of `count` floats per rank into recv[world * count], rank-major.  0 = success. */
typedef int (*dpe_allgather_fn)(void* user, const float* send, size_t count, float* recv);
/* The same all-gather on DEVICE buffers of the pipeline's GPU (RCCL over xGMI in the CLI); the hook
 * returns once recv is complete.  With the default runner the depth maps then go from each rank's
 * HBM-resident state to the others' without a host copy. */
typedef int (*dpe_allgather_dev_fn)(void* user, const float* dev_send, size_t count, float* dev_recv);
/* Optional: called once when one of this rank's collectives failed, before dpe_run_pipeline returns,
 * so that peers blocked in theirs fail fast (bin/dpe: ncclCommAbort).  Return value ignored. */
typedef int (*dpe_abort_fn)(void* user);

/* Fusion projection tests of one reference view: same contract as dpe_fusion_candidates
 * (include/dpe_mvs.h) over the given views (the default runs the HIP kernel on gpu_index).
 * Threading: the callback may be invoked from a thread other than the caller of dpe_run_pipeline
 * (the pipeline fetches the next image's candidates on a worker thread while it fuses the current
 * one), and never concurrently with itself: one call returns before the next begins.  So the
 * callee must not rely on per-thread state set up by an earlier call or by the pipeline's caller --
 * the current device of the HIP runtime and a per-thread last-error slot are such state: select
 * the device in every call and return errors through the return value (the default runner does). */
typedef int (*dpe_fusion_fn)(void* user, const DpeFusionView* views, int n_views, int ref, const int* src, int ns,
                             int32_t* idx, float* val);

enum { DPE_SCHEDULE_REFERENCE = 0, DPE_SCHEDULE_JACOBI = 1 };

typedef struct DpePipelineOptions {
  int gpu_index;            /* device of the default runner */
  bool verbose, fusion, viz, depth, normal, weak, edge;   /* RunDPEPipeline's flags */
  int schedule;             /* DPE_SCHEDULE_*: reference = serial order (later images see this
                               pass's depths of earlier ones); jacobi = depths of the previous pass */
  int rank, world_size;     /* problems are split in contiguous blocks; world > 1 forces jacobi */
  dpe_allgather_fn allgather; void* allgather_user;   /* required when world_size > 1 */
  dpe_pass_runner_fn runner; void* runner_user;       /* NULL: libdpe_mvs on gpu_index */
  uint64_t base_seed;       /* Philox key of image i: base_seed ^ (i * 0x9E3779B97F4A7C15) */
  bool keep_intermediate;   /* also write depths.dmb / normals.dmb / weak.bin / selected_views.bin and
                               keep edges_<s>.dmb / labels_<s>.dmb (the reference deletes them) */
  dpe_fusion_fn fusion_runner; void* fusion_user;     /* NULL: the HIP kernel on gpu_index */
  int max_iterations;       /* PatchMatch iterations per pass; 0 = the reference's 3 (main.cpp:527, 554) */
  bool photometric_only;    /* geom_consistency = false on every pass (BASELINE config 2; the
                               reference always runs its geometric passes, main.cpp:549) */
  dpe_allgather_dev_fn allgather_device; void* allgather_device_user;   /* optional (see above); with the
                               default runner it is used instead of `allgather` for the depth maps */
  dpe_abort_fn abort_collectives; void* abort_user;   /* optional (see dpe_abort_fn) */
  int fusion_mode;          /* DPE_FUSION_ETH3D (0, the default): RunFusion, what RunDPEPipeline calls;
                               DPE_FUSION_TAT_INTERMEDIATE / DPE_FUSION_TAT_ADVANCED: the Tanks-and-Temples
                               variants (DPE.cpp:1372-1689), whole image on the GPU; with a fusion_runner
                               hook (no GPU) their serial loops run on the host and the hook is not called.
                               Any other value fails */
  int point_cloud;          /* 0 (the default): off.  DPE_POINTS_ALL (1) / DPE_POINTS_STRONG (2): after the last
                               pass of every resolution round ((iteration + 1) % 4 == 0, main.cpp:456) every
                               reference image's point_<iteration>.ply goes into its result folder
                               (ExportDepthImagePointCloud; 2: STRONG pixels only, main.cpp:464).  Independent
                               of `viz`, under which the reference nests it.  Any other value fails */
  int consistency;          /* 0 (the default): off.  1..255 = min_views: every reference image's result folder gets
                               consistency.npy (|u1 [H][W]: the source views of its pair.txt line that pass
                               RunFusion's reprojection, depth and angle tests at the pixel, without RunFusion's
                               masks and blocks) and depth_filtered.npy (<f4 [H][W]: the final depth where that
                               count >= min_views, else 0), from the final maps, independent of the depth / normal
                               flags; each rank writes its own images.  On the GPU (dpe_fusion_consistency), or
                               with a fusion_runner hook on host threads (dpe_host_consistency): the same files.
                               Must be the same on every rank.  Any other value fails */
} DpePipelineOptions;

void dpe_pipeline_default_options(DpePipelineOptions* opt);
/* RunDPEPipeline: 0 on success, nonzero on failure (message in dpe_pipeline_last_error()). */
int dpe_run_pipeline(const char* dense_folder, const DpePipelineOptions* opt);
const char* dpe_pipeline_last_error(void);
/* Wall seconds of the last successful dpe_run_pipeline on this process: [0] total, [1] image decode,
 * [2] the GetProblemEdges pre-pass (EdgeSegment), [3] the passes (with the depth exchanges),
 * [4] outputs + fusion, [5] the depth exchanges alone (multi-rank: status all-gather, export,
 * all-gather, import, summed over the pass rounds; 0 for one rank), [6] the pass work alone (each
 * pass round up to its GPU work's end, on one rank too), [7] RunFusion (part of [4]; with several
 * ranks it includes the exchange of the final normals / pixel states; 0 without fusion), [8] the
 * consistency maps (part of [4]: views, filter and files of this rank's images; with several ranks and
 * no fusion it includes that exchange; 0 without `consistency`).  Returns the number of entries
 * written (<= n, at most 9). */
int dpe_pipeline_last_timings(double* out, int n);

/* Grey-level decode of a JPEG (baseline/extended, luma plane) or binary PGM.  Writes up to `cap`
 * bytes into `out` (pass NULL/0 to query the size) and the size into *w, *h.  0 on success. */
int dpe_host_read_gray(const char* path, uint8_t* out, size_t cap, int* w, int* h);
/* Colour decode (cv::imread IMREAD_COLOR): 8-bit BGR, up to `cap` bytes; size query with out = NULL. */
int dpe_host_read_bgr(const char* path, uint8_t* out, size_t cap, int* w, int* h);
/* ReadCamera (DPE.cpp:341-382): extrinsic, intrinsic, "dmin interval num dmax" line.  0 on success. */
int dpe_host_read_camera(const char* path, DpeCamera* cam);
/* cv::resize INTER_LINEAR of a CV_32FC1 image (float weights, horizontal then vertical pass). */
void dpe_host_resize_linear(const float* src, int w, int h, float* dst, int nw, int nh);
/* RescaleMatToTargetSize: nearest with the reference's swapped factors; `elem` bytes per pixel;
 * destination pixels whose source falls outside keep their (caller-initialised) value. */
void dpe_host_rescale_nearest(const void* src, int w, int h, void* dst, int nw, int nh, int elem);

/* EdgeSegment (DPE.cpp:129-291): mode 0 = edges (uint8 0/255, same size as src, use_canny = 1 in the
 * reference's call), mode 1 = labels (int32: -1 small region, 0 boundary, > 0 region; size
 * round(src / 2^scale), use_canny = 0).  Writes up to `cap` bytes into `out` (NULL: size query via
 * *ow, *oh).  0 on success. */
int dpe_host_edge_segment(int scale, const uint8_t* src, int w, int h, int mode, int use_canny, int high_res, void* out,
                          size_t cap, int* ow, int* oh);
/* EdgeSegment's labels (mode 1, use_canny = 0) together with its img_connect picture (DPE.cpp:256-290,
 * connect_<s>.jpg of the viz medium results), from one segmentation: 8-bit BGR colors[label] of every
 * pixel taken BEFORE the small regions become -1.  The colour is a fixed 32-bit hash of the label
 * (label 0 black), where the reference draws from an unseeded rand().  labels / connect_bgr hold
 * cap_pixels pixels (both NULL: size query).  0 on success. */
int dpe_host_edge_segment_connect(int scale, const uint8_t* src, int w, int h, int high_res, int32_t* labels,
                                  uint8_t* connect_bgr, size_t cap_pixels, int* ow, int* oh);
/* cv::Canny(src, dst, low, high, 3, L2gradient = true): dst uint8 0/255.  0 on success. */
int dpe_host_canny(const uint8_t* src, int w, int h, double low, double high, uint8_t* dst);
/* cv::resize(INTER_LINEAR) of a CV_8UC1 image (exact 1/2: INTER_AREA fast path).  0 on success. */
int dpe_host_resize_u8(const uint8_t* src, int w, int h, uint8_t* dst, int nw, int nh);
/* Connect (DPE.cpp:27-127): labels of the 4-connected zero regions (255 -> 0); returns the label
 * count (label_cnt entries, written up to cnt_cap) or -1. */
int dpe_host_connect(const uint8_t* img, int w, int h, int* label, int* cnt, int cnt_cap);
/* cv::HoughLinesP: writes up to `cap` segments (x0, y0, x1, y1) into `lines`; returns the count or -1. */
int dpe_host_hough_lines_p(const uint8_t* img, int w, int h, double rho, double theta, int threshold, double min_len,
                           double max_gap, int* lines, int cap);

/*
 * Baseline JPEG encoder: what cv::imwrite(path, mat) writes with its defaults (libjpeg, baseline
 * sequential, Annex K Huffman tables, JFIF APP0; channels = 3: 8-bit BGR as Y/Cb/Cr 4:2:0,
 * channels = 1: one component).  Integer arithmetic; split where the GPU takes over:
 *   dpe_host_jpeg_blocks        front half: pixels -> quantised coefficient blocks in scan (MCU) order.
 *                               Colour: 16x16 MCUs in raster order, blocks Y00 Y01 Y10 Y11 Cb Cr; grey:
 *                               one block per 8x8 MCU.  64 int16 per block in NATURAL (row-major) order,
 *                               not zigzag.  Writes up to `cap` int16 values (blocks = NULL: size query);
 *                               *n_blocks receives the block count.  dpe_state_render_jpeg_blocks
 *                               (dpe_mvs.h) computes the same blocks on the device.
 *   dpe_host_jpeg_write_blocks  back half: DC prediction, Huffman coding, byte stuffing, headers, file.
 *   dpe_host_write_jpeg         the two chained.
 * 0 on success.
 */
int dpe_host_jpeg_blocks(const uint8_t* pixels, int w, int h, int channels, int quality, int16_t* blocks, size_t cap,
                         size_t* n_blocks);
int dpe_host_jpeg_write_blocks(const char* path, const int16_t* blocks, int w, int h, int channels, int quality);
int dpe_host_write_jpeg(const char* path, const uint8_t* pixels, int w, int h, int channels, int quality);
/* ShowDepthMap / ShowNormalMap / ShowWeakImage (DPE.cpp:384-502) of a w x h state into 8-bit BGR
 * [h][w][3]: `kind` = DPE_VIZ_DEPTH (reads depth f32 [h][w], depth_min, depth_max), DPE_VIZ_NORMAL
 * (normal f32 [h][w][3]) or DPE_VIZ_WEAK (weak u8 [h][w]); the other inputs may be NULL.  0 on success. */
int dpe_host_viz_render(int kind, int w, int h, const float* depth, const float* normal, const uint8_t* weak,
                        float depth_min, float depth_max, uint8_t* bgr);

/*
 * The Tanks-and-Temples fusions as the reference writes them (DPE.cpp:1372-1689): the serial loops,
 * with the per-view entries that are never reset between pixels.  The yardstick of
 * dpe_fusion_tat_image (dpe_mvs.h) and what fusion_mode runs without a GPU.
 *   dpe_host_fusion_tat_serial      fuses views[0..n-1] in order, `mode` = DPE_FUSION_TAT_*; src_ids are
 *                                   image ids (pair.txt order); bgr u8 [H][W][3]; block u8 [H][W] or NULL;
 *                                   mask (u8 [H][W], or NULL) receives the view's final fusion mask.
 *                                   Writes up to `cap` points and returns their number, or -1.
 *   dpe_host_fusion_tat_run         the same views through the path dpe_run_pipeline takes: gpu_index < 0
 *                                   the serial loops (= dpe_host_fusion_tat_serial), else every image on
 *                                   that device (stage, begin, one dpe_fusion_tat_image per view, in a
 *                                   context of its own); `mask` is filled by the serial loops only.
 *                                   tools/fusion_prof.py times one against the other.
 *   dpe_host_fusion_tat_thresholds  D[k], k = 2..n-1: the smallest float in [-1, 1] whose GetAngle is
 *                                   below the Intermediate angle threshold at k (what the device test
 *                                   `dot >= D[k]` needs).  0, or nonzero when the table does not verify.
 *   dpe_host_fusion_tat_angle_test  the serial loop's own test: GetAngle(dot) < k * 3 deg + 4 deg.
 */
typedef struct DpeHostTatView {
  int image_id;
  const int* src_ids;
  int n_src;
  DpeFusionView view;
  const uint8_t* bgr;
  const uint8_t* block;
  uint8_t* mask;
} DpeHostTatView;
long long dpe_host_fusion_tat_serial(int mode, const DpeHostTatView* views, int n, DpeFusedPoint* out, size_t cap);
long long dpe_host_fusion_tat_run(int mode, const DpeHostTatView* views, int n, int gpu_index, DpeFusedPoint* out,
                                  size_t cap);
int dpe_host_fusion_tat_thresholds(float* D, int n);
int dpe_host_fusion_tat_angle_test(float dot, int k);

/*
 * ExportDepthImagePointCloud (DPE.cpp:1691-1724) as the reference writes it: the serial double loop,
 * columns outside and rows inside, over HOST arrays that are already at the map size (depth f32 [h][w],
 * weak u8 [h][w] PixelState, NULL allowed in DPE_POINTS_ALL, bgr u8 [h][w][3]).  `mode`, the test and the
 * point are dpe_state_point_cloud's (dpe_mvs.h), whose yardstick this is, and what point_cloud runs
 * without a GPU.  Writes up to `cap` points; returns their number, or -1 for a bad argument or when
 * `cap` is too small.
 *   dpe_host_rescale_image_and_camera  RescaleImageAndCamera (DPE.cpp:1123-1144): the src_w x src_h BGR
 *                                   image resized to w x h per channel (dpe_host_resize_u8) into
 *                                   `out_bgr`, and cam->K[0], K[2] *= w / (float)src_w, K[4], K[5] *=
 *                                   h / (float)src_h; equal sizes copy the image and leave K alone.
 *   dpe_host_write_point_cloud      ExportPointCloud (DPE.cpp:532-572): binary little-endian PLY, xyz
 *                                   float + BGR uchar.  0 on success.
 */
long long dpe_host_depth_point_cloud(int mode, int w, int h, const float* depth, const uint8_t* weak, const DpeCamera* cam,
                                     const uint8_t* bgr, float depth_min, float depth_max, DpeFusedPoint* out, size_t cap);
int dpe_host_rescale_image_and_camera(const uint8_t* bgr, int src_w, int src_h, int w, int h, DpeCamera* cam,
                                      uint8_t* out_bgr);
int dpe_host_write_point_cloud(const char* path, const DpeFusedPoint* points, size_t n);

/*
 * The consistency maps (DpePipelineOptions.consistency) on the host: the yardstick of
 * dpe_fusion_consistency (dpe_mvs.h, which states the tests) and what the option runs without a GPU.
 *   dpe_host_consistency                the serial double loop over reference view `ref` of views[0..n_views-1]
 *                                       against src[0..ns-1] (indices into views), calling acosf itself:
 *                                       count u8 [H][W], depth_filtered f32 [H][W] (either may be NULL).
 *                                       0, or nonzero for what dpe_fusion_consistency refuses.
 *   dpe_host_consistency_dot_threshold  *D = the smallest float in [-1, 1] whose acosf is below 0.174533f
 *                                       (what the device test `dot >= D` needs), found and verified as
 *                                       dpe_host_fusion_tat_thresholds does.  0, or nonzero when it does not verify.
 *   dpe_host_consistency_angle_test     the loop's own test: GetAngle(dot) < 0.174533f.
 */
int dpe_host_consistency(const DpeFusionView* views, int n_views, int ref, const int* src, int ns, int min_views,
                         uint8_t* count, float* depth_filtered);
int dpe_host_consistency_dot_threshold(float* D);
int dpe_host_consistency_angle_test(float dot);

/*
 * Cloud evaluation: precision, recall and F-score of a reconstructed cloud against a ground-truth cloud.
 * No counterpart in the reference.  The numbers are those of the two clouds as given: no registration,
 * cropping or down-sampling (dpe_host_cloud_eval_prep below adds a crop box and voxel down-sampling,
 * dpe_host_cloud_eval_reg a rigid registration before them), so they are not a benchmark's leaderboard figures.
 *   dpe_host_cloud_nn          the contract of dpe_cloud_nn (dpe_mvs.h: d2, truncation at R2 = R*R, non-finite
 *                              points) over the same grid on host threads (at most 16): the same bits.  The
 *                              yardstick of the device path and the path used without a GPU.
 *   dpe_host_read_point_cloud  the vertex positions of a PLY, `ascii` or `binary_little_endian 1.0`: scalar
 *                              properties x, y, z of the `vertex` element at any position, float or double
 *                              (rounded to float); other scalar properties are skipped by their size, later
 *                              elements ignored.  Writes up to `cap` points into xyz f32 [cap][3] and their
 *                              number into *n (xyz = NULL: the number only).  A list property inside `vertex`,
 *                              a big-endian file, a truncated body, a count above 2^31 - 1 and a missing
 *                              coordinate fail.  Reads what dpe_host_write_point_cloud writes.
 *   dpe_host_cloud_eval        a = out(recon -> gt), c = out(gt -> recon) at radius R (0: the largest tau);
 *                              1 <= n_tau <= 16, every tau finite with 0 < tau <= R.
 *                                precision[k] = #{ i : a[i] < tau[k]*tau[k] } / n_recon   (product in float,
 *                                recall[k]    = the same from c over n_gt                  division in double;
 *                                fscore[k]    = 2 p r / (p + r), 0 when p + r = 0          0 for an empty cloud)
 *                                mean_*_truncated = sum of sqrt((double)a[i]) / n in index order: means of
 *                                distances truncated at R, not of the distances themselves.
 *                              Points with a non-finite coordinate are counted in dropped_* and still count in
 *                              the denominators.  gpu_index < 0: dpe_host_cloud_nn; else dpe_cloud_nn_pair in a
 *                              context of its own on that device.  The counts and means are taken on the host
 *                              from the distance arrays on both paths: equal structs.
 * Each returns 0, or nonzero with the message in dpe_pipeline_last_error().
 */
#define DPE_CLOUD_MAX_TAU 16
typedef struct DpeCloudEval {
  int n_tau;
  float radius;                         /* the R that was used */
  float tau[DPE_CLOUD_MAX_TAU];
  double precision[DPE_CLOUD_MAX_TAU], recall[DPE_CLOUD_MAX_TAU], fscore[DPE_CLOUD_MAX_TAU];
  double mean_accuracy_truncated, mean_completeness_truncated;
  unsigned long long n_recon, n_gt, dropped_recon, dropped_gt;
} DpeCloudEval;
int dpe_host_cloud_nn(const float* query, size_t n, const float* target, size_t m, float radius, float* d2_out);
int dpe_host_read_point_cloud(const char* path, float* xyz, size_t cap, size_t* n);
int dpe_host_cloud_eval(const float* recon, size_t n, const float* gt, size_t m, const float* tau, int n_tau, float radius,
                        int gpu_index, DpeCloudEval* out);

/*
 * Preparing clouds for the evaluation, and thinning one: crop box and voxel down-sampling.
 *   dpe_host_cloud_voxel           the contract of dpe_cloud_voxel (dpe_mvs.h: cell, lattice centroid, colour
 *                                  mean rounded half up, first, count, ascending `first`) as a serial loop with
 *                                  a hash map over the same header functions (csrc/cloud_dist.h): the same
 *                                  bits.  The yardstick of the device path and the path used without a GPU.
 *                                  A voxel holding one point may return that point moved by one float ulp.
 *                                  More voxels than `cap`: nonzero, *k = their number, nothing written.
 *   dpe_host_cloud_crop            keeps the points that are finite and have lo[a] <= p[a] <= hi[a] on every
 *                                  axis, compared as floats (both ends inclusive), in their order; colours (u8
 *                                  [n][3], or NULL) are carried along.  Writes the kept points, colours and
 *                                  original indices (each output may be NULL) and returns their number; the
 *                                  outputs hold n entries at most.
 *   dpe_host_read_point_cloud_rgb  dpe_host_read_point_cloud plus the three `uchar` colour properties a PLY of
 *                                  ours carries, diffuse_blue / diffuse_green / diffuse_red or blue / green /
 *                                  red, into rgb u8 [cap][3] as (b, g, r).  *has_rgb = 1 when the file has all
 *                                  three, else 0 and rgb is left alone.  The refusals are the same.
 *   dpe_host_cloud_eval_prep       dpe_host_cloud_eval after a preparation: both clouds are cropped to the box
 *                                  first (use_crop != 0), then down-sampled (voxel > 0; 0 = none), then scored.
 *                                  gpu_index >= 0 runs the down-sampling on that device in the same context as
 *                                  the distances; both paths fill equal structs.  n_recon and n_gt of
 *                                  DpeCloudEval are the counts AFTER the preparation; the counts before it come
 *                                  back in prep->n_recon_in and prep->n_gt_in.  prep = NULL is
 *                                  dpe_host_cloud_eval unchanged.
 * dpe_host_cloud_crop returns a count; the others 0, or nonzero with the message in dpe_pipeline_last_error().
 */
typedef struct DpeCloudPrep {
  float voxel;                          /* voxel edge; 0: no down-sampling */
  int use_crop;                         /* nonzero: keep crop_lo <= p <= crop_hi */
  float crop_lo[3], crop_hi[3];
  unsigned long long n_recon_in, n_gt_in;   /* out: the counts before the preparation */
} DpeCloudPrep;
int dpe_host_cloud_voxel(const float* xyz, size_t n, const uint8_t* rgb_or_null, float voxel, float* out_xyz,
                         uint8_t* out_rgb, int32_t* out_first, int32_t* out_count, size_t cap, size_t* k);
size_t dpe_host_cloud_crop(const float* xyz, size_t n, const uint8_t* rgb_or_null, const float* lo, const float* hi,
                           float* out_xyz, uint8_t* out_rgb, int32_t* out_index);
int dpe_host_read_point_cloud_rgb(const char* path, float* xyz, uint8_t* rgb, size_t cap, size_t* n, int* has_rgb);
int dpe_host_cloud_eval_prep(const float* recon, size_t n, const float* gt, size_t m, const float* tau, int n_tau, float radius,
                             int gpu_index, DpeCloudPrep* prep, DpeCloudEval* out);

/*
 * Rigid registration of a source cloud to a target cloud: point-to-point ICP over the nearest neighbour with
 * index (dpe_mvs.h states both contracts).  No counterpart in the reference.
 *   dpe_host_cloud_nn_index   the contract of dpe_cloud_nn_index over dpe_host_cloud_nn's grid on host threads
 *                             (at most 16): the same indices and bits.
 *   dpe_host_cloud_icp_step   one step (dpe_cloud_icp_step's contract) with the pairwise tree taken literally:
 *                             the yardstick of the device step.
 *   dpe_host_cloud_transform  out[i] = the image of xyz[i] under T (12 doubles, row-major 3 x 4), the x'
 *                             expression of the step; a non-finite point becomes NaN on every axis.  out may be
 *                             xyz.
 *   dpe_host_cloud_solve      the absolute transform of the ORIGINAL source points from one step's sums, N =
 *                             matched >= 3: means sum(a)/N and sum(b)/N, H = sum(ab) - sum(a) sum(b)^T / N, the
 *                             rotation from Horn's unit quaternion (the eigenvector of the 4 x 4 symmetric matrix
 *                             of H with the largest eigenvalue, cyclic Jacobi in double, sqrt the only libm call),
 *                             always a proper rotation; t = (o_t + mean b) - R (o_s + mean a).  Host only, and
 *                             what both paths of dpe_host_cloud_register call.
 *   dpe_host_cloud_register   the loop.  radius[0 .. n_radii): 1 to 4 stages, each finite and > 0, run in the
 *                             given order (coarse to fine); per stage at most max_iters steps (1..1000), each
 *                             followed by the solve, so nothing is composed from step to step.  rms =
 *                             sqrt(sum(d2) / N).  A stage ends after a step whose sums and count equal the
 *                             previous step's bit for bit (converged = 2, a fixed point), else when
 *                             |rms - rms_prev| <= tol * rms_prev (converged = 1; tol >= 0), else at max_iters
 *                             (converged = 0).  Starts from init (use_init != 0) or the identity.  Fewer than 3
 *                             matches in a step fail ("fewer than 3 matches within the radius").  gpu_index < 0:
 *                             dpe_host_cloud_icp_step; else dpe_cloud_icp_stage / dpe_cloud_icp_step in a context
 *                             of its own on that device: equal structs.  On failure *out is not written.
 *   dpe_host_cloud_eval_reg   dpe_host_cloud_eval_prep after a registration of the reconstruction to the ground
 *                             truth: with prep->voxel > 0 the voxel-down-sampled copies of both clouds are
 *                             registered, and the ground truth is cropped first when prep has a box (the
 *                             reconstruction is not: the box is in the ground truth's frame); then the WHOLE
 *                             reconstruction is transformed and scored exactly as dpe_host_cloud_eval_prep scores
 *                             it (prep may be NULL).  Everything on gpu_index runs in one context.
 * Each returns 0, or nonzero with the message in dpe_pipeline_last_error().
 */
#define DPE_CLOUD_MAX_RADII 4
typedef struct DpeCloudRegOptions {
  float radius[DPE_CLOUD_MAX_RADII];
  int n_radii;
  int max_iters;
  double tol;
  int use_init;
  double init[12];
} DpeCloudRegOptions;
typedef struct DpeCloudReg {
  double T[12];
  int stages;
  int iters[DPE_CLOUD_MAX_RADII];
  long long matched[DPE_CLOUD_MAX_RADII];
  double rms[DPE_CLOUD_MAX_RADII];
  int converged[DPE_CLOUD_MAX_RADII];
} DpeCloudReg;
int dpe_host_cloud_nn_index(const float* query, size_t n, const float* target, size_t m, float radius, float* d2_out,
                            int32_t* idx_out);
int dpe_host_cloud_icp_step(const float* src, size_t n, const float* tgt, size_t m, float radius, const double* T,
                            DpeIcpSums* out);
int dpe_host_cloud_transform(const double* T, const float* xyz, size_t n, float* out);
int dpe_host_cloud_solve(const DpeIcpSums* sums, const double* o_s, const double* o_t, double* T);
int dpe_host_cloud_register(const float* src, size_t n, const float* tgt, size_t m, const DpeCloudRegOptions* opt,
                            int gpu_index, DpeCloudReg* out);
int dpe_host_cloud_eval_reg(const float* recon, size_t n, const float* gt, size_t m, const float* tau, int n_tau, float radius,
                            int gpu_index, DpeCloudPrep* prep_or_null, const DpeCloudRegOptions* opt, DpeCloudReg* reg,
                            DpeCloudEval* out);

/*
 * Depth-map evaluation: the estimated maps DPE/%08d/depth.npy of a dense folder against a ground-truth scan
 * rendered into each view, or against ground-truth maps.  No counterpart in the reference.  dpe_mvs.h states the
 * contract of the render and the score (dpe_cloud_render_view, dpe_depth_score).
 *   dpe_host_cloud_render   that render as a loop over the points on the host (csrc/depth_eval.h's arithmetic;
 *                           large scans are split over host threads, each with a z-buffer of its own, and the
 *                           buffers merged by minimum, which no order can change): the device path's bits.
 *   dpe_host_depth_score    that score as a serial loop over the pixels with the pairwise tree taken literally:
 *                           the device path's bits, struct and error map (err_or_null).
 *   dpe_host_depth_stats    everything derived, in double, for both paths: accuracy[k] = within[k] / n_both,
 *                           completeness[k] = within[k] / n_gt, mae = sum_abs / n_both, mre = sum_rel / n_both,
 *                           rmse = sqrt(sum_sq / n_both); 0 where the denominator is 0.
 *   dpe_host_read_npy_f32   a 2-D '<f4' .npy v1.0 in C order (what the pipeline writes): data == NULL gives the
 *                           size only; another version, dtype, rank or order, a body shorter or longer than the
 *                           header says and cap < w * h fail.
 *   dpe_host_depth_eval_list  the image ids of `dense_folder` in ascending order: the folders DPE/%08d that hold
 *                           `map_name` (NULL: "depth.npy").  ids == NULL or cap too small: *n only.
 *   dpe_host_depth_eval     every listed image scored, rows[i] in ascending id, and their total (the integers add,
 *                           the three doubles are added sequentially in that order).  gt_maps_dir ==
 *                           NULL: the scan gt_xyz (n_gt points) is rendered into cams/%08d_cam.txt, its
 *                           intrinsics scaled from the size of images/%08d.jpg to the map's (the arithmetic of the
 *                           consistency maps' views), with half-width `splat`; else gt_maps_dir/%08d.npy is the
 *                           ground truth and must have the map's size.  write_maps: depth_gt.npy and
 *                           depth_error.npy beside each map.  gpu_index < 0: the host functions above; else
 *                           the scan is staged once in a context of that device and every view rendered and
 *                           scored there: equal rows.  cap < the number of images fails.
 * All return 0, or nonzero with the message in dpe_pipeline_last_error().
 */
typedef struct DpeDepthStats {
  double accuracy[DPE_DEPTH_MAX_TAU], completeness[DPE_DEPTH_MAX_TAU], mae, mre, rmse;
} DpeDepthStats;
typedef struct DpeDepthEvalOptions {
  const char* dense_folder;
  const char* map_name;       /* NULL: "depth.npy" */
  const char* gt_maps_dir;    /* NULL: render the scan */
  int splat, mode, n_tau;
  float tau[DPE_DEPTH_MAX_TAU];
  int write_maps, gpu_index;
} DpeDepthEvalOptions;
typedef struct DpeDepthImage {
  int id, width, height;
  DpeDepthScore score;
} DpeDepthImage;
int dpe_host_cloud_render(const float* xyz, size_t n, const DpeCamera* cam, int splat, float* depth_out);
int dpe_host_depth_score(const float* est, const float* gt, int w, int h, const float* tau, int n_tau, int mode,
                         DpeDepthScore* out, float* err_or_null);
void dpe_host_depth_stats(const DpeDepthScore* s, int n_tau, DpeDepthStats* out);
int dpe_host_read_npy_f32(const char* path, float* data, size_t cap, int* w, int* h);
int dpe_host_depth_eval_list(const char* dense_folder, const char* map_name, int* ids, size_t cap, size_t* n);
int dpe_host_depth_eval(const DpeDepthEvalOptions* opt, const float* gt_xyz, size_t n_gt, DpeDepthImage* rows, size_t cap,
                        size_t* n_rows, DpeDepthScore* total);

/*
 * Normal-map evaluation: the estimated maps DPE/%08d/normal.npy of a dense folder against the normals of a
 * ground-truth scan (estimated by PCA over each point's radius neighbourhood) rendered into each view, or against
 * ground-truth normal maps.  No counterpart in the reference.  dpe_mvs.h states the contract of the three parts
 * (dpe_cloud_normals, dpe_cloud_render_view_normals, dpe_normal_score); csrc/normal_eval.h holds their arithmetic.
 *   dpe_host_cloud_normals         the point normals over dpe_host_cloud_nn's grid on host threads (at most 16), a cell
 *                                  of the 27 skipped when an earlier one gave its bucket: the device path's bits,
 *                                  counts and sums.
 *   dpe_host_cloud_render_normals  the render with winners as a loop over the points (64-bit words bits(z) << 32 |
 *                                  index, their minimum per pixel): depth map and world-frame normal map, either may
 *                                  be NULL.
 *   dpe_host_normal_score          the score as a serial loop over the pixels with the pairwise tree taken literally.
 *   dpe_host_normal_edges          E[0..180): the bin edges (float)cos(b degrees), THE function both paths use.
 *   dpe_host_normal_cos            a threshold in degrees as the cosine the score takes: (float)cos((double)deg * pi /
 *                                  180), the one place where degrees become cosines.
 *   dpe_host_normal_stats          everything derived, in double, for both paths and both programs: share[k] =
 *                                  within[k] / n_both, completeness[k] = within[k] / n_gt, mean_cos_dist = sum_dist /
 *                                  n_both, and from the histogram to its 1 degree resolution, a pixel of bin b counted
 *                                  at b + 0.5 degrees: mean_deg, and median_deg of the first bin at which the
 *                                  cumulative count reaches half of n_both; 0 where the denominator is 0.
 *   dpe_host_read_npy_f32x3        dpe_host_read_npy_f32 for a 3-D '<f4' [h][w][3]; the same refusals.
 *   dpe_host_normal_eval           dpe_host_depth_eval's folder walk over normal.npy (map_name NULL): rows in ascending
 *                                  id and their total (the integers add, the two doubles are added sequentially in
 *                                  that order).  gt_maps_dir == NULL: the normals of the scan gt_xyz are estimated once
 *                                  (radius, min_nb), staged with it and rendered into every view at the map's size
 *                                  (the depth tool's camera rule); else gt_maps_dir/%08d.npy [h][w][3] is the ground
 *                                  truth.  write_maps: normal_gt.npy and normal_error.npy beside each map.  gpu_index <
 *                                  0: the host functions above; else everything in one context of that device: equal
 *                                  rows.
 * All return 0, or nonzero with the message in dpe_pipeline_last_error().
 * Left out: a DpePipelineOptions field, reading or writing a PLY with normals, curvature or planarity output.
 */
typedef struct DpeNormalStats {
  double share[DPE_NORMAL_MAX_TAU], completeness[DPE_NORMAL_MAX_TAU], mean_cos_dist, median_deg, mean_deg;
} DpeNormalStats;
typedef struct DpeNormalEvalOptions {
  const char* dense_folder;
  const char* map_name;       /* NULL: "normal.npy" */
  const char* gt_maps_dir;    /* NULL: estimate and render the scan's normals */
  float radius;               /* of the PCA neighbourhood */
  int min_nb, splat, n_tau;
  float cos_tau[DPE_NORMAL_MAX_TAU];
  int write_maps, gpu_index;
} DpeNormalEvalOptions;
typedef struct DpeNormalImage {
  int id, width, height;
  DpeNormalScore score;
} DpeNormalImage;
int dpe_host_cloud_normals(const float* xyz, size_t n, float radius, int min_nb, float* normal_out, int32_t* count_out,
                           long long* sums_out_or_null);
int dpe_host_cloud_render_normals(const float* xyz, const float* normals, size_t n, const DpeCamera* cam, int splat,
                                  float* depth_out_or_null, float* normal_out_or_null);
int dpe_host_normal_score(const float* est, const float* gt, int w, int h, const float* cos_tau, int n_tau,
                          DpeNormalScore* out, float* err_or_null);
void dpe_host_normal_edges(float* edges);
float dpe_host_normal_cos(double deg);
void dpe_host_normal_stats(const DpeNormalScore* s, int n_tau, DpeNormalStats* out);
int dpe_host_read_npy_f32x3(const char* path, float* data, size_t cap, int* w, int* h);
int dpe_host_normal_eval(const DpeNormalEvalOptions* opt, const float* gt_xyz, size_t n_gt, DpeNormalImage* rows, size_t cap,
                         size_t* n_rows, DpeNormalScore* total);

#ifdef __cplusplus
}
#endif
#endif /* DPE_HOST_H_ */
