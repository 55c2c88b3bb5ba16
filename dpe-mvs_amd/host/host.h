// host.h — internal interfaces of the host pipeline (libdpe_host.so).  Plain C++17, no HIP: the
// device work goes through the C-ABI of dpe_mvs.h.
#pragma once
#include <array>
#include <cstdint>
#include <mutex>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/dpe_host.h"
#include "../csrc/fusion_world.h"   // FP3, fz_world, fz_pixel, fz_pair, fz_dot: the arithmetic shared with the kernels

namespace dpe_host {

struct GrayImage {
  int w = 0, h = 0;
  std::vector<uint8_t> px;
};
struct ColorImage {                 // cv::imread(IMREAD_COLOR): 8-bit BGR, row-major
  int w = 0, h = 0;
  std::vector<uint8_t> bgr;
};
bool decode_jpeg(const uint8_t* data, size_t size, bool color, GrayImage* gray, ColorImage* bgr, std::string& err);
bool decode_jpeg_luma(const uint8_t* data, size_t size, GrayImage& img, std::string& err);
bool decode_jpeg_bgr(const uint8_t* data, size_t size, ColorImage& img, std::string& err);
bool read_gray(const std::string& path, GrayImage& img, std::string& err);
bool read_bgr(const std::string& path, ColorImage& img, std::string& err);

// cv::Mat as the .dmb files carry it: OpenCV type code + raw rows (DPE.cpp:293-339)
enum { CV_8UC1 = 0, CV_8SC1 = 1, CV_32SC1 = 4, CV_32FC1 = 5, CV_32FC3 = 21 };
struct Mat {
  int rows = 0, cols = 0, type = CV_8UC1;
  std::vector<uint8_t> data;
  static int elem_size(int type);
  void create(int r, int c, int t) { rows = r; cols = c; type = t; data.assign((size_t)r * c * elem_size(t), 0); }
  template <class T> T* ptr() { return reinterpret_cast<T*>(data.data()); }
  template <class T> const T* ptr() const { return reinterpret_cast<const T*>(data.data()); }
  bool empty() const { return rows == 0 || cols == 0; }
};
bool read_bin_mat(const std::string& path, Mat& m, std::string& err);
bool write_bin_mat(const std::string& path, const Mat& m, std::string& err);
// .npy v1.0 (main.cpp:47-96); descr "<f4" / "|i1" / "|u1"
bool write_npy(const std::string& path, const void* data, const std::vector<int64_t>& shape, const char* descr,
               size_t elem, std::string& err);
// a 2-D '<f4' .npy v1.0 in C order, h rows of w; anything else (another version or dtype, Fortran order, another
// rank, a body shorter or longer than the header says) is refused with a message
bool read_npy_f32(const std::string& path, std::vector<float>& data, int& w, int& h, std::string& err);

bool read_camera(const std::string& path, DpeCamera& cam, std::string& err);   // DPE.cpp:341-382

void resize_linear(const float* src, int w, int h, float* dst, int nw, int nh);
void rescale_nearest(const void* src, int w, int h, void* dst, int nw, int nh, int elem);

std::string fmt_index(int i);   // ToFormatIndex: %08d

// edges.cpp: EdgeSegment and the OpenCV operations it uses (DPE.cpp:9-291, main.cpp:331-388)
void resize_u8(const uint8_t* src, int w, int h, uint8_t* dst, int nw, int nh);
void threshold_binary(uint8_t* img, size_t n, int thr);
void canny_l2(const uint8_t* src, int w, int h, double low, double high, uint8_t* dst);
void roberts(const uint8_t* src, int w, int h, uint8_t* dst);
void connect(const uint8_t* img, int w, int h, int* label, std::vector<int>& label_cnt);
void draw_line(uint8_t* img, int w, int h, int x0, int y0, int x1, int y1, uint8_t value);
void hough_lines_p(const uint8_t* img, int w, int h, double rho, double theta, int threshold, double min_len,
                   double max_gap, std::vector<std::array<int, 4>>& lines);
// The device for EdgeSegment's data-parallel stages (dpe_resize_linear / dpe_resize_u8 / dpe_canny /
// dpe_roberts_threshold, bit-identical to the host functions above): one context shared by the host
// threads behind `mu`.  ctx == nullptr: every stage on the host.
struct EdgeDevice {
  DpeContext* ctx = nullptr;
  std::mutex* mu = nullptr;
};
// `connect_bgr` (mode 1 only): also returns img_connect (DPE.cpp:267-284), colors[label] of every
// pixel before the small regions become -1, 8-bit BGR of the labels' size
bool edge_segment(int scale, const uint8_t* src, int cols, int rows, int mode, bool use_canny, bool high_res, Mat& out,
                  std::string& err, const EdgeDevice* dev = nullptr, std::vector<uint8_t>* connect_bgr = nullptr);
// `viz`: also writes rawedge_<s>.jpg / connect_<s>.jpg beside a map it computes (main.cpp:361-364, 380-383)
bool get_problem_edges(const GrayImage& full, int scale_size, const std::string& result_folder, bool use_edge,
                       bool use_label, bool high_res, std::string& err, const EdgeDevice* dev = nullptr, bool viz = false);

// jpeg_enc.cpp: baseline JPEG encoder (cv::imwrite's defaults), split into the front half
// (pixels -> quantised blocks in scan order, natural coefficient order) and the back half
size_t jpeg_block_count(int w, int h, int channels);
void jpeg_blocks(const uint8_t* px, int w, int h, int channels, int quality, int16_t* blocks);
void jpeg_encode_blocks(const int16_t* blocks, int w, int h, int channels, int quality, std::vector<uint8_t>& file);
bool jpeg_write_blocks(const std::string& path, const int16_t* blocks, int w, int h, int channels, int quality,
                       std::string& err);
bool write_jpeg(const std::string& path, const uint8_t* px, int w, int h, int channels, int quality, std::string& err);

// viz.cpp: ShowDepthMap / ShowNormalMap / ShowWeakImage (DPE.cpp:384-502) into 8-bit BGR
void viz_render(int kind, int w, int h, const float* depth, const float* normal, const uint8_t* weak, float dmin,
                float dmax, uint8_t* bgr);
void connect_color(int label, uint8_t* bgr);

// fusion.cpp: RunFusion (DPE.cpp:1220-1370) / ExportPointCloud (DPE.cpp:532-572)
struct FusionView {
  int image_id = 0;
  std::vector<int> src_ids;          // pair.txt order
  DpeFusionView view{};              // size, camera, depth, normal (borrowed pointers)
  const uint8_t* weak = nullptr;     // PixelState [H][W]
  std::vector<uint8_t> bgr;          // colour image at the map size
  std::vector<uint8_t> block;        // blocks/mask_<id>.jpg at the map size, or empty
  std::vector<uint8_t> mask;         // fusion masks (set by run_fusion)
};
using FusedPoint = DpeFusedPoint;   // x, y, z, b, g, r
bool run_fusion(std::vector<FusionView>& views, dpe_fusion_fn fn, void* user, std::vector<FusedPoint>& cloud,
                std::string& err);
// fz_world with the colour packed in: the point a fused pixel contributes
inline FusedPoint fusion_point(int x, int y, float depth, const DpeCamera& cam, const float* bgr) {
  const dpe::FP3 X = dpe::fz_world(x, y, depth, cam);
  return FusedPoint{X.x, X.y, X.z, bgr[0], bgr[1], bgr[2]};
}
// The problems as indices into the views, by the reference's imageIdToindexMap: emplace keeps the first of equal
// ids, operator[] gives 0 for an unknown one.  `images`: (image id, source ids) of every view, in view order; the
// plan covers the problems `mine` (indices into `images`), or all of them.  The limits on the number of sources
// stay with the callers.
struct FusionPlan {
  std::vector<int> refs;
  std::vector<std::vector<int>> srcs;
  bool aliased = false;   // a reference among its own sources, or an image id twice
  using Image = std::pair<int, const std::vector<int>*>;
  explicit FusionPlan(const std::vector<Image>& images, const std::vector<int>* mine = nullptr) {
    std::unordered_map<int, int> index;
    for (size_t i = 0; i < images.size(); ++i)
      if (!index.emplace(images[i].first, (int)i).second) aliased = true;
    auto idx_of = [&](int id) { auto it = index.find(id); return it == index.end() ? 0 : it->second; };
    const size_t n = mine ? mine->size() : images.size();
    refs.resize(n); srcs.resize(n);
    for (size_t k = 0; k < n; ++k) {
      const Image& im = images[mine ? (size_t)(*mine)[k] : k];
      refs[k] = idx_of(im.first);
      for (int id : *im.second) {
        srcs[k].push_back(idx_of(id));
        if (srcs[k].back() == refs[k]) aliased = true;
      }
    }
  }
};
FusionPlan fusion_plan(const std::vector<FusionView>& views);   // fusion.cpp: the plan of every view
// a host range page-locked for its lifetime when the runtime allows (dpe_host_pin); a refusal is silent: the range
// stays pageable and everything still works
struct PinnedRange {
  void* p = nullptr;
  void pin(void* q, size_t bytes) { if (dpe_host_pin(q, bytes) == DPE_OK) p = q; }
  PinnedRange() = default;
  ~PinnedRange() { if (p) dpe_host_unpin(p); }
  PinnedRange(const PinnedRange&) = delete;
  PinnedRange& operator=(const PinnedRange&) = delete;
};
bool export_point_cloud(const std::string& path, const FusedPoint* cloud, size_t n, std::string& err);
bool export_point_cloud(const std::string& path, const std::vector<FusedPoint>& cloud, std::string& err);
// points.cpp: RescaleImageAndCamera (DPE.cpp:1123-1144) and ExportDepthImagePointCloud (DPE.cpp:1691-1724)
void scale_intrinsics(DpeCamera& cam, float sx, float sy);   // K of an image resized by (sx, sy)
// `img` resized to w x h per channel (resize_u8) into `bgr`, and cam's intrinsics scaled with it
void resize_bgr_and_camera(const ColorImage& img, int w, int h, DpeCamera& cam, std::vector<uint8_t>& bgr);
// the serial double loop, columns outside: the number of points, or -1 when `cap` is too small
long long depth_point_cloud(int mode, int w, int h, const float* depth, const uint8_t* weak, const DpeCamera& cam,
                            const uint8_t* bgr, float depth_min, float depth_max, FusedPoint* out, size_t cap);
// fusion_tat.cpp: RunFusion_TAT_Intermediate / RunFusion_TAT_advanced (DPE.cpp:1372-1689), `mode` =
// DPE_FUSION_TAT_*.  ctx == nullptr: the reference's serial loops on the host; else every image on
// the device (the serial loops still run when a reference is among its own sources or an id repeats).
bool run_fusion_tat(std::vector<FusionView>& views, int mode, DpeContext* ctx, std::vector<FusedPoint>& cloud,
                    std::string& err);
// D[k], k = 2..n-1: smallest dot product in [-1, 1] that passes the Intermediate angle test at k
bool tat_thresholds(float* D, int n, std::string& err);
// what every fusion loop is written with: Get3DPointonWorld, ProjectCamera, the source pixel of a projection and the
// pair arithmetic are csrc/fusion_world.h's (fz_*); GetAngle from the dot product (DPE.cpp:1208-1217) and the
// smallest float D in [-1, 1] with get_angle(D) < T (bisection on the float's bits, verified at D and at its
// predecessor) are fusion_tat.cpp's, the only callers of acos
using dpe::FP3; using dpe::FzPair; using dpe::fz_world; using dpe::fz_pixel; using dpe::fz_pair; using dpe::fz_dot;
float get_angle(float dot_product);
enum class DotThreshold { kOk, kNonePasses, kUnverified };
DotThreshold angle_dot_threshold(float T, float& D);
// consistency.cpp: the consistency maps (RunFusion's view loop, DPE.cpp:1312-1343, without the masks and
// the blocks): the serial double loop over reference view `ref` of `views`, src = indices into `views`.
// count u8 [H][W] and filtered f32 [H][W] may be null.
void consistency_image(const DpeFusionView* views, int ref, const int* src, int ns, int min_views, uint8_t* count,
                       float* filtered);
bool consistency_dot_threshold(float& D, std::string& err);
// the arguments dpe_host_consistency refuses, as dpe_fusion_consistency does (the message into err)
bool consistency_args_ok(int n_views, int ref, const int* src, int ns, int min_views, std::string& err);

// pipeline.cpp: the message dpe_pipeline_last_error returns on this thread (the helpers of cloud_eval.cpp and
// ply_read.cpp report through it)
void set_last_error(const std::string& msg);
// the extern "C" form of a host function: 0, or 1 with its message (`otherwise` when it left none) for
// dpe_pipeline_last_error
template <class F>
int c_entry(F&& run, const char* otherwise = "") {
  std::string err = otherwise;
  if (run(err)) return 0;
  set_last_error(err);
  return 1;
}
// The context of a tool that runs on either path: none for gpu_index < 0 (the host path), else one of its own on that
// device, destroyed with the owner.  A failed dpe_create leaves ok false and err = who + ": " + dpe_last_error()
struct OwnedContext {
  DpeContext* ctx = nullptr;
  bool ok = true;
  OwnedContext(int gpu_index, const char* who, std::string& err) {
    if (gpu_index < 0) return;
    ctx = dpe_create(gpu_index);
    ok = ctx != nullptr;
    if (!ok) err = std::string(who) + ": " + dpe_last_error();
  }
  ~OwnedContext() { if (ctx) dpe_destroy(ctx); }
  OwnedContext(const OwnedContext&) = delete;
  OwnedContext& operator=(const OwnedContext&) = delete;
};
// dpe_last_error() in the host path's wording, so both paths report alike: the device entry's name in front gives
// way to the host function's
inline std::string device_error(const char* who, const char* entry) {
  std::string msg = dpe_last_error();
  const std::string lead = std::string(entry) + ": ";
  if (msg.compare(0, lead.size(), lead) == 0) msg = msg.substr(lead.size());
  return std::string(who) + ": " + msg;
}
// cloud_eval.cpp: the truncated nearest-neighbour distance of dpe_cloud_nn (dpe_mvs.h) over the same grid
// (csrc/cloud_dist.h) on host threads, and the evaluation built on it (gpu_index < 0: that path, else
// dpe_cloud_nn_pair in a context of its own; the counts and means on the host either way)
bool cloud_nn(const float* query, size_t n, const float* target, size_t m, float radius, float* out, std::string& err);
bool cloud_eval(const float* recon, size_t n, const float* gt, size_t m, const float* tau, int n_tau, float radius,
                int gpu_index, DpeCloudEval* out, std::string& err);
// ply_read.cpp: the vertex positions of an ascii / binary little-endian PLY; xyz == nullptr: *n only
bool read_point_cloud(const std::string& path, float* xyz, size_t cap, size_t* n, std::string& err);
// the same with the file's three uchar colours as (b, g, r) in rgb[3 * i ...]; *has_rgb = 0 and rgb untouched for a
// file without them
bool read_point_cloud_rgb(const std::string& path, float* xyz, uint8_t* rgb, size_t cap, size_t* n, int* has_rgb,
                          std::string& err);
// cloud_eval.cpp: cloud_eval over a context the caller owns (nullptr: on host threads)
bool cloud_eval_in(DpeContext* ctx, const float* recon, size_t n, const float* gt, size_t m, const float* tau, int n_tau,
                   float radius, DpeCloudEval* out, std::string& err);
// cloud_voxel.cpp: the voxel down-sampling of dpe_cloud_voxel (dpe_mvs.h) as a serial loop over the same
// arithmetic (csrc/cloud_dist.h); false with more voxels than `cap` (*k = their number, nothing written) and
// for what dpe_cloud_voxel refuses
bool cloud_voxel(const float* xyz, size_t n, const uint8_t* rgb, float voxel, float* out_xyz, uint8_t* out_rgb,
                 int32_t* out_first, int32_t* out_count, size_t cap, size_t* k, std::string& err);
// the indices of the finite points with lo[a] <= p[a] <= hi[a] on every axis, ascending
void cloud_crop(const float* xyz, size_t n, const float lo[3], const float hi[3], std::vector<int32_t>& keep);
// crop (optional) and down-sampling (voxel > 0) of both clouds, then cloud_eval_in: gpu_index >= 0 runs the
// down-sampling and the distances in one context on that device
bool cloud_eval_prep(const float* recon, size_t n, const float* gt, size_t m, const float* tau, int n_tau, float radius,
                     int gpu_index, DpeCloudPrep* prep, DpeCloudEval* out, std::string& err);
// what cloud_eval_prep refuses in its clouds and its block before any work (the message into err)
bool cloud_prep_args(const float* recon, size_t n, const float* gt, size_t m, const DpeCloudPrep& prep, std::string& err);
// one cloud through the preparation (crop when `crop`, then voxel > 0) into pts; ctx or nullptr as above
bool cloud_prepare(DpeContext* ctx, const float* xyz, size_t n, const DpeCloudPrep& prep, bool crop, std::vector<float>& pts,
                   std::string& err);
// cloud_eval_prep after the checks, over a context the caller owns (nullptr: on the host)
bool cloud_eval_prep_in(DpeContext* ctx, const float* recon, size_t n, const float* gt, size_t m, const float* tau, int n_tau,
                        float radius, DpeCloudPrep* prep, DpeCloudEval* out, std::string& err);
// cloud_eval.cpp: the nearest neighbour with its index (dpe_cloud_nn_index of dpe_mvs.h) over cloud_nn's grid
bool cloud_radius_ok(float radius);
bool cloud_nn_index(const float* query, size_t n, const float* target, size_t m, float radius, float* out, int32_t* idx,
                    std::string& err);
// cloud_register.cpp: one ICP step, the solve and the loop (dpe_host.h states them); register_in runs over a context
// the caller owns (nullptr: the host step)
bool cloud_icp_step(const float* src, size_t n, const float* tgt, size_t m, float radius, const double* T, DpeIcpSums* out,
                    std::string& err);
bool cloud_solve(const DpeIcpSums& s, const double* o_s, const double* o_t, double* T, std::string& err);
bool cloud_register_in(DpeContext* ctx, const float* src, size_t n, const float* tgt, size_t m, const DpeCloudRegOptions& opt,
                       DpeCloudReg* out, std::string& err);
// depth_eval.cpp: the render of a scan into one view and the score of one map (dpe_cloud_render_view and
// dpe_depth_score of dpe_mvs.h) as loops over the same arithmetic (csrc/depth_eval.h; the loops both map evaluations
// share are map_eval.h's) and what is derived from a score
bool cloud_render(const float* xyz, size_t n, const DpeCamera& cam, int splat, float* out, std::string& err);
bool depth_score(const float* est, const float* gt, int w, int h, const float* tau, int n_tau, int mode, DpeDepthScore* out,
                 float* errmap, std::string& err);
void depth_stats(const DpeDepthScore& s, int n_tau, DpeDepthStats* out);
// what the folder tools share: the image ids DPE/<8 digits> of `dense` that hold `map`, ascending (`who` leads the
// message), and the camera of image `id` at the size w x h of its map (map_view's arithmetic)
bool eval_list(const char* who, const std::string& dense, const std::string& map, std::vector<int>& ids, std::string& err);
bool map_camera(const std::string& dense, int id, int w, int h, DpeCamera& cam, std::string& err);
// a 3-D '<f4' .npy v1.0 in C order, [h][w][3]; refusals as read_npy_f32's
bool read_npy_f32x3(const std::string& path, std::vector<float>& data, int& w, int& h, std::string& err);
// normal_eval.cpp: the normal-map evaluation (dpe_cloud_normals, dpe_cloud_render_view_normals and dpe_normal_score of
// dpe_mvs.h) as loops over the same arithmetic (csrc/normal_eval.h) and what is derived from a score
bool cloud_normals(const float* xyz, size_t n, float radius, int min_nb, float* normal, int32_t* count, long long* sums,
                   std::string& err);
bool cloud_render_normals(const float* xyz, const float* normals, size_t n, const DpeCamera& cam, int splat, float* depth,
                          float* normal, std::string& err);
bool normal_score(const float* est, const float* gt, int w, int h, const float* cos_tau, int n_tau, DpeNormalScore* out,
                  float* errmap, std::string& err);
void normal_stats(const DpeNormalScore& s, int n_tau, DpeNormalStats* out);

}  // namespace dpe_host
