// pipeline.cpp — RunDPEPipeline (main.cpp:474-600) over the C-ABI PatchMatch pass.
//
// Kept from the reference: the dense_folder contract (images/%08d.jpg, cams/%08d_cam.txt, pair.txt
// in; DPE/%08d/ results; edges_<s>.dmb / labels_<s>.dmb read from the result folders), the
// coarse-to-fine schedule and its per-pass parameters (main.cpp:490-570), InuputInitialization's
// rescaling rules (DPE.cpp:733-914), the ProcessProblem epilogue (main.cpp:423-446) and the final
// .npy outputs (main.cpp:99-260).
//
// Different by design: every image is decoded once and its pyramid levels cached; per-image state
// (depth, normal, weak, selected views) stays in memory between passes instead of .dmb round
// trips; problems are split in contiguous blocks over ranks (one process per GPU) and the depth
// maps are all-gathered after every pass; "reference" schedule = the reference's serial order,
// "jacobi" = each pass reads the previous pass's depths (forced when world_size > 1).
//
// GetProblemEdges (main.cpp:331-388) runs before the first pass as in the reference: edges_<s>.dmb /
// labels_<s>.dmb that are missing are computed by EdgeSegment (edges.cpp) and written.
// fusion = true runs RunFusion (fusion.cpp) on rank 0 after the outputs: the per-(pixel, view)
// projection tests on the GPU (dpe_fusion_candidates), the order-dependent rest on the host; with
// several ranks the final normals and pixel states are all-gathered first.  fusion_mode selects the
// reference's two Tanks-and-Temples fusions instead (fusion_tat.cpp): one image at a time on the GPU,
// or, with a fusion_runner hook, their serial loops on the host.  As in the reference the
// edges_/labels_ maps are deleted at the end unless keep_intermediate.
//
// viz = true writes the reference's medium results: depth_<it>.jpg / normal_<it>.jpg / weak_<it>.jpg
// after every pass (main.cpp:448-454; <it> = the 0-based pass index) and rawedge_<s>.jpg /
// connect_<s>.jpg beside the maps GetProblemEdges computes.  With the default runner the pictures
// are rendered and taken through the data-parallel half of the JPEG encode on the GPU from the
// HBM-resident state (dpe_state_render_jpeg_blocks); only the quantised blocks come back, into a
// few pinned buffers, and a small pool of host threads (VizWriter) Huffman-codes and writes them
// while the following passes run.  With a runner hook the state is on the host and the same
// pictures come from viz.cpp / jpeg_enc.cpp, byte for byte the same files.
//
// point_cloud = 1 / 2 writes the reference's per-image point clouds (ExportDepthImagePointCloud, whose
// call is the commented block at main.cpp:456-466): point_<it>.ply after the last pass of every
// resolution round, from the post-epilogue state, 2 = STRONG pixels only (main.cpp:464).  An option of
// its own here (the reference nests it under the medium results).  With the default runner the points
// are computed from the HBM-resident state (dpe_state_point_cloud) and only they come back, into two
// pinned buffers that a host thread (PointCloudWriter) encodes and writes while the following passes
// run; with a runner hook dpe_host_depth_point_cloud's loop runs on the host state.  Same files.
//
// consistency = min_views (1..255) writes, for every reference image, consistency.npy (how many source
// views of its pair.txt line pass RunFusion's reprojection, depth and angle tests at each pixel, without
// RunFusion's order-dependent masks and without the blocks) and depth_filtered.npy (the final depth where
// that count reaches min_views).  It reads what fusion reads, the final maps of every image, so the same
// gather feeds it, and then every rank filters its own images: on the GPU (dpe_fusion_consistency over
// the staged views, which ETH3D fusion in the same context reuses; 5 bytes per pixel come back), or, with
// a fusion_runner hook, dpe_host_consistency on host threads.  Same files.  Only cameras are read for it.
//
// run() at the end of the file is the table of contents: the phases of a run in order, each a
// member of PipelineRun.  The rule every phase keeps with several ranks is in rank_group.h.
#include "host.h"
#include "parallel.h"
#include "rank_group.h"
#include "viz_writer.h"
#include "point_writer.h"

#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <map>
#include <memory>
#include <sstream>

namespace fs = std::filesystem;

namespace dpe_host {
namespace {

thread_local std::string g_err;
const char* kOutName = "DPE";
// dpe_pipeline_last_timings: wall seconds of the last run's phases
enum TimeSlot {
  kTimeTotal = 0,
  kTimeDecode,     // image decode, up to the first GetProblemEdges
  kTimeEdges,      // the GetProblemEdges pre-pass
  kTimePasses,     // the passes, incl. the exchanges
  kTimeOutputs,    // outputs + fusion
  kTimeExchange,   // (multi-rank) the depth exchanges alone
  kTimePassWork,   // the pass work alone
  kTimeFusion,     // RunFusion alone (rank 0, incl. the normal/weak exchange that feeds it)
  kTimeConsistency,   // the consistency maps alone (incl. that exchange when there is no fusion)
  kNumTimes
};
static_assert(kNumTimes == 9, "include/dpe_host.h documents entries [0]..[8]");
double g_times[kNumTimes] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Problem {   // main.h:108-118
  int index = 0, ref_image_id = 0;
  std::vector<int> src_image_ids;
  std::string dense_folder, result_folder;
  int scale_size = 1;
  DpePatchMatchParams params;
  int iteration = 0;
};

struct DepthMap { int w = 0, h = 0; std::vector<float> d; };

struct ImageState {   // depths.dmb / normals.dmb / weak.bin / selected_views.bin of one image
  int w = 0, h = 0;
  std::vector<float> depth, normal;     // normal: [h][w][3]
  std::vector<uint8_t> weak;
  std::vector<uint32_t> sel;
};

int std_round(float v) { return (int)std::round(v); }   // std::round: half away from zero

std::string image_path(const std::string& dense, int id) { return (fs::path(dense) / "images" / (fmt_index(id) + ".jpg")).string(); }
std::string cam_path(const std::string& dense, int id) { return (fs::path(dense) / "cams" / (fmt_index(id) + "_cam.txt")).string(); }

bool generate_sample_list(const std::string& dense, std::vector<Problem>& probs, std::string& err) {   // main.cpp:264-308
  std::ifstream f(fs::path(dense) / "pair.txt");
  if (!f) { err = "cannot read pair.txt in " + dense; return false; }
  std::string line;
  std::getline(f, line);
  int n = 0;
  std::istringstream(line) >> n;
  for (int i = 0; i < n; ++i) {
    Problem p;
    dpe_params_default(&p.params);
    p.index = i;
    std::getline(f, line);
    std::istringstream(line) >> p.ref_image_id;
    p.dense_folder = dense;
    p.result_folder = (fs::path(dense) / kOutName / fmt_index(p.ref_image_id)).string();
    std::error_code ec;
    fs::create_directories(p.result_folder, ec);
    std::getline(f, line);
    std::istringstream is(line);
    int m = 0;
    is >> m;
    for (int j = 0; j < m; ++j) {
      int id; float score;
      is >> id >> score;
      if (score <= 0.0f) continue;
      p.src_image_ids.push_back(id);
    }
    probs.push_back(std::move(p));
  }
  return true;
}

class ImageCache {
 public:
  explicit ImageCache(std::string folder) : folder_(std::move(folder)) {}
  const std::vector<float>* full(int idx, int& w, int& h, std::string& err) {
    auto it = full_.find(idx);
    if (it == full_.end()) {
      GrayImage g;
      if (!read_gray(image_path(folder_, idx), g, err)) return nullptr;
      Level L{g.w, g.h, std::vector<float>(g.px.begin(), g.px.end())};
      it = full_.emplace(idx, std::move(L)).first;
    }
    w = it->second.w; h = it->second.h;
    return &it->second.px;
  }
  // decodes the images not cached yet on host threads (independent files; same pixels as full())
  bool prefetch(const std::vector<int>& ids, std::string& err) {
    std::vector<int> todo;
    for (int id : ids)
      if (!full_.count(id) && std::find(todo.begin(), todo.end(), id) == todo.end()) todo.push_back(id);
    std::vector<GrayImage> g(todo.size());
    std::vector<std::string> e(todo.size());
    const int nt = std::max(1, std::min<int>(host_threads(), (int)todo.size()));
    run_on_threads(nt, [&](int t) {
      for (size_t k = t; k < todo.size(); k += nt) read_gray(image_path(folder_, todo[k]), g[k], e[k]);
    });
    for (size_t k = 0; k < todo.size(); ++k) {
      if (!e[k].empty()) { err = e[k]; return false; }
      full_.emplace(todo[k], Level{g[k].w, g[k].h, std::vector<float>(g[k].px.begin(), g[k].px.end())});
    }
    return true;
  }
  const std::vector<float>* level(int idx, int scale, int& w, int& h, std::string& err) {
    int fw, fh;
    const std::vector<float>* f = full(idx, fw, fh, err);
    if (!f) return nullptr;
    if (scale == 1) { w = fw; h = fh; return f; }
    const auto key = std::make_pair(idx, scale);
    auto it = lvl_.find(key);
    if (it == lvl_.end()) {
      const float factor = 1.0f / (float)scale;
      const int nw = std_round(fw * factor), nh = std_round(fh * factor);
      Level L{nw, nh, std::vector<float>((size_t)nw * nh)};
      resize_linear(f->data(), fw, fh, L.px.data(), nw, nh);
      it = lvl_.emplace(key, std::move(L)).first;
    }
    w = it->second.w; h = it->second.h;
    return &it->second.px;
  }

 private:
  struct Level { int w, h; std::vector<float> px; };
  std::string folder_;
  std::map<int, Level> full_;
  std::map<std::pair<int, int>, Level> lvl_;
};

int scale_index(int scale_size) { int s = 0; while ((1 << s) < scale_size) s++; return s; }

void pass_params(DpePatchMatchParams& p, int i, int j) {   // main.cpp:510-556 (j = -1: first pass of round i)
  if (j < 0) {
    if (i == 0) { p.state = DPE_FIRST_INIT; p.use_APD = false; p.use_edge = false; }
    else {
      p.state = DPE_REFINE_INIT; p.use_APD = true; p.use_edge = true;
      p.ransac_threshold = (float)(0.01 - i * 0.00125);
      p.rotate_time = std::min((int)std::pow(2, i), 4);
    }
    p.geom_consistency = false;
    p.max_iterations = 3;
    p.weak_peak_radius = 6;
  } else {
    p.state = DPE_REFINE_ITER;
    p.use_APD = i != 0; p.use_edge = i != 0;
    p.ransac_threshold = (float)(0.01 - i * 0.00125);
    p.rotate_time = std::min((int)std::pow(2, i), 4);
    p.geom_consistency = true;
    p.max_iterations = 3;
    p.weak_peak_radius = std::max(4 - 2 * j, 2);
  }
}

template <class T>
std::vector<T> rescaled(const std::vector<T>& src, int w, int h, int nw, int nh, int ch = 1) {
  if (w == nw && h == nh) return src;
  std::vector<T> dst((size_t)nw * nh * ch, T(0));
  rescale_nearest(src.data(), w, h, dst.data(), nw, nh, (int)sizeof(T) * ch);
  return dst;
}

bool read_support(const Problem& p, const std::string& name, Mat& m, std::string& err) {
  const std::string path = (fs::path(p.result_folder) / name).string();
  if (!fs::exists(path)) {
    err = path + " missing (GetProblemEdges writes it before the first pass)";
    return false;
  }
  return read_bin_mat(path, m, err);
}

struct Runner {
  dpe_pass_runner_fn fn = nullptr;
  void* user = nullptr;
  DpeContext* ctx = nullptr;
  ~Runner() { if (ctx) dpe_destroy(ctx); }
};
int native_runner(void* user, const DpePassInput* in, const DpePassState* st) {
  return dpe_pm_run(static_cast<DpeContext*>(user), in, st);
}

struct NativeFusion {
  DpeContext* ctx = nullptr;
  bool own = false;
  std::vector<DpeFusionView> staged;   // what the context holds: the same views (sizes, cameras, maps) stage once
  std::string err;   // the library's message of a failed call (run_fusion calls from a worker thread,
                     // and dpe_last_error() is per thread)
  ~NativeFusion() { if (own && ctx) dpe_destroy(ctx); }
  int stage(const DpeFusionView* views, int n) {
    static_assert(sizeof(DpeFusionView) == 2 * sizeof(int) + sizeof(DpeCamera) + 2 * sizeof(void*), "compared as bytes");
    if ((int)staged.size() == n && std::memcmp(staged.data(), views, (size_t)n * sizeof(DpeFusionView)) == 0) return DPE_OK;
    staged.clear();
    const int r = dpe_fusion_stage(ctx, views, n);
    if (r != DPE_OK) { err = dpe_last_error(); return r; }
    staged.assign(views, views + n);
    return DPE_OK;
  }
};
int native_fusion(void* user, const DpeFusionView* views, int n, int ref, const int* src, int ns, int32_t* idx,
                  float* val) {
  NativeFusion* f = static_cast<NativeFusion*>(user);
  if (const int r = f->stage(views, n); r != DPE_OK) return r;
  const int r = dpe_fusion_candidates(f->ctx, ref, src, ns, idx, val);
  if (r != DPE_OK) f->err = dpe_last_error();
  return r;
}

// the per-pass intermediate maps of the reference (main.cpp:439-446)
bool write_state_maps(const Problem& p, const ImageState& s, std::string& err) {
  const struct { const char* name; int type; const void* data; } maps[4] = {
      {"depths.dmb", CV_32FC1, s.depth.data()}, {"normals.dmb", CV_32FC3, s.normal.data()},
      {"weak.bin", CV_8UC1, s.weak.data()}, {"selected_views.bin", CV_32SC1, s.sel.data()}};
  Mat m;
  for (const auto& e : maps) {
    m.create(s.h, s.w, e.type);
    std::memcpy(m.data.data(), e.data, m.data.size());
    if (!write_bin_mat((fs::path(p.result_folder) / e.name).string(), m, err)) return false;
  }
  return true;
}

// host copy of an image's HBM-resident state (depth_only: a state imported from another rank)
bool fetch_state(DpeContext* ctx, int id, ImageState& s, std::string& err, bool depth_only = false) {
  int w = 0, h = 0;
  if (dpe_state_fetch(ctx, id, &w, &h, nullptr, nullptr, nullptr, nullptr) != 0) { err = dpe_last_error(); return false; }
  const size_t L = (size_t)w * h;
  s.w = w; s.h = h;
  s.depth.resize(L);
  if (!depth_only) { s.normal.resize(L * 3); s.weak.resize(L); s.sel.resize(L); }
  const int rc = dpe_state_fetch(ctx, id, &w, &h, s.depth.data(), depth_only ? nullptr : s.normal.data(),
                                 depth_only ? nullptr : s.weak.data(), depth_only ? nullptr : s.sel.data());
  if (rc != 0) { err = dpe_last_error(); return false; }
  return true;
}

std::string viz_path(const Problem& p, int kind) {   // depth_<it>.jpg / normal_<it>.jpg / weak_<it>.jpg
  return (fs::path(p.result_folder) / (kVizNames[kind] + std::to_string(p.iteration) + ".jpg")).string();
}

// One pass's DpePassInput and the storage its pointers borrow (the decode cache owns the pixels).
struct PassInput {
  std::vector<int> ids;   // the reference image, then its source views
  std::vector<const float*> images;
  std::vector<DpeCamera> cams;
  Mat edge, edge_low, label;
  int W = 0, H = 0;
  DpePassInput in;
};

// InuputInitialization + SupportInitialization (DPE.cpp:733-914, 1025-1052): cameras and level
// images, the depth range (into p.params), the support maps, seed and salt.  in.depths stays null.
bool build_pass_input(Problem& p, ImageCache& cache, uint64_t base_seed, PassInput& pi, std::string& err) {
  DpePatchMatchParams& P = p.params;
  pi.ids.assign(1, p.ref_image_id);
  pi.ids.insert(pi.ids.end(), p.src_image_ids.begin(), p.src_image_ids.end());
  if ((int)pi.ids.size() > DPE_MAX_IMAGES) { err = "Can't process so much images: " + std::to_string(pi.ids.size()); return false; }
  int fw, fh;
  if (!cache.full(pi.ids[0], fw, fh, err)) return false;
  pi.cams.resize(pi.ids.size());
  for (size_t k = 0; k < pi.ids.size(); ++k) {
    DpeCamera& cam = pi.cams[k];
    if (!read_camera(cam_path(p.dense_folder, pi.ids[k]), cam, err)) return false;
    int w, h;
    const std::vector<float>* img = cache.level(pi.ids[k], p.scale_size, w, h, err);
    if (!img) return false;
    if (p.scale_size != 1) scale_intrinsics(cam, w / (float)fw, h / (float)fh);
    cam.width = w; cam.height = h;   // scale 1: the full size
    if (k == 0) { pi.W = w; pi.H = h; }
    pi.images.push_back(img->data());
  }
  const int W = pi.W, H = pi.H;
  P.depth_min = pi.cams[0].depth_min * 0.6f;
  P.depth_max = pi.cams[0].depth_max * 1.2f;
  P.num_images = (int)pi.ids.size();
  DpePassInput& in = pi.in;
  std::memset(&in, 0, sizeof(in));
  in.width = W; in.height = H; in.num_images = (int)pi.ids.size();
  in.images = pi.images.data();
  in.cams = pi.cams.data();
  if (P.use_edge || P.use_limit) {
    const int s = scale_index(p.scale_size);
    const int max_s = P.high_res_img ? scale_index(P.max_scale_size) : s;
    if (!read_support(p, "edges_" + std::to_string(s) + ".dmb", pi.edge, err)) return false;
    if (!read_support(p, "edges_" + std::to_string(max_s) + ".dmb", pi.edge_low, err)) return false;
    if (pi.edge.rows != H || pi.edge.cols != W || pi.edge.type != CV_8UC1) { err = "edge map size/type mismatch in " + p.result_folder; return false; }
    in.edge = pi.edge.ptr<uint8_t>();
    in.edge_low_res = pi.edge_low.ptr<uint8_t>();
    in.low_width = pi.edge_low.cols; in.low_height = pi.edge_low.rows;
  }
  if (P.use_label) {
    if (!read_support(p, "labels_" + std::to_string(scale_index(p.scale_size)) + ".dmb", pi.label, err)) return false;
    if (pi.label.rows != H || pi.label.cols != W || pi.label.type != CV_32SC1) { err = "label map size/type mismatch in " + p.result_folder; return false; }
    in.label = pi.label.ptr<int32_t>();
  }
  in.params = P;
  in.seed = base_seed ^ ((uint64_t)p.ref_image_id * 0x9E3779B97F4A7C15ull);
  in.pass_salt = (uint32_t)p.iteration;
  in.image_ids = pi.ids.data();        // pyramid levels stay in HBM across passes (keyed by id and size)
  return true;
}

bool write_outputs(const Problem& p, const ImageState& s, const DpePipelineOptions& opt, std::string& err) {   // main.cpp:572-578
  const std::vector<int64_t> hw{s.h, s.w};
  const fs::path rf(p.result_folder);
  if (opt.depth) {
    std::vector<float> d = s.depth;
    for (size_t i = 0; i < d.size(); ++i) if (s.weak[i] == DPE_UNKNOWN) d[i] = 0.0f;   // ZeroDepthForUnknown
    if (!write_npy((rf / "depth.npy").string(), d.data(), hw, "<f4", 4, err)) return false;
  }
  if (opt.normal && !write_npy((rf / "normal.npy").string(), s.normal.data(), {s.h, s.w, 3}, "<f4", 4, err)) return false;
  if (opt.weak) {
    std::vector<int8_t> e(s.weak.size());
    for (size_t i = 0; i < e.size(); ++i) e[i] = s.weak[i] == DPE_WEAK ? 1 : (s.weak[i] == DPE_STRONG ? 2 : 0);
    if (!write_npy((rf / "weak.npy").string(), e.data(), hw, "|i1", 1, err)) return false;
  }
  if (opt.edge) {
    for (int idx = 0; idx < 8; ++idx) {
      const fs::path ep = rf / ("edges_" + std::to_string(idx) + ".dmb");
      if (!fs::exists(ep)) continue;
      Mat m;
      if (!read_bin_mat(ep.string(), m, err)) return false;
      std::vector<int8_t> b(m.data.size());
      for (size_t i = 0; i < b.size(); ++i) b[i] = m.data[i] > 0 ? 1 : 0;
      if (!write_npy((rf / "edge.npy").string(), b.data(), {m.rows, m.cols}, "|i1", 1, err)) return false;
      break;
    }
  }
  return true;
}

// The maps of problem `p`'s final state `st` (borrowed) and its camera at their size: ReadCamera, with
// the intrinsics scaled as RescaleImageAndCamera (DPE.cpp:1123-1144) scales them for a src_w x src_h
// image.  No image is read: all the consistency maps need of a view.
bool map_view(const Problem& p, const ImageState& st, int src_w, int src_h, DpeFusionView& view, std::string& err) {
  DpeCamera cam;
  if (!read_camera(cam_path(p.dense_folder, p.ref_image_id), cam, err)) return false;
  if (src_w != st.w || src_h != st.h) scale_intrinsics(cam, st.w / (float)src_w, st.h / (float)src_h);
  cam.width = st.w; cam.height = st.h;
  view.width = st.w; view.height = st.h;
  view.cam = cam;
  view.depth = st.depth.data();
  view.normal = st.normal.data();
  return true;
}

// One fusion view: map_view, the colour image (decode + RescaleImageAndCamera) and the block mask of
// problem `p` at the size of its final state `st`.
bool load_fusion_view(const Problem& p, const ImageState& st, bool use_block, FusionView& v, std::string& err) {
  v.image_id = p.ref_image_id;
  v.src_ids = p.src_image_ids;
  ColorImage img;
  if (!read_bgr(image_path(p.dense_folder, p.ref_image_id), img, err)) return false;
  if (!map_view(p, st, img.w, img.h, v.view, err)) return false;
  if (img.w != st.w || img.h != st.h) {   // RescaleImageAndCamera's image half (map_view has scaled the camera)
    DpeCamera scratch = v.view.cam;
    resize_bgr_and_camera(img, st.w, st.h, scratch, v.bgr);
  } else {
    v.bgr = std::move(img.bgr);
  }
  if (use_block) {
    GrayImage b;
    if (!read_gray((fs::path(p.dense_folder) / "blocks" / ("mask_" + std::to_string(p.ref_image_id) + ".jpg")).string(), b, err)) return false;
    if (b.w != st.w || b.h != st.h) { err = "block mask size differs from the depth map"; return false; }
    v.block = std::move(b.px);
  }
  v.weak = st.weak.data();
  return true;
}

// The state of one dpe_run_pipeline call and its phases, in the order run() calls them.  A phase
// returns false when the run ends there with `err` set.  With several ranks a phase's own failure
// is not such an end: it raises the rank's flag (ranks.fail) and the rank goes on joining the
// collectives, doing no more work (rank_group.h).
struct PipelineRun {
  PipelineRun(const std::string& dense_folder, const DpePipelineOptions& o, std::string& e)
      : opt(o), dense(dense_folder), err(e), ranks(o), cache(dense_folder),
        jacobi(ranks.multi() || o.schedule == DPE_SCHEDULE_JACOBI) {}

  const DpePipelineOptions& opt;
  const std::string dense;
  std::string& err;
  RankGroup ranks;
  std::vector<Problem> problems;
  ImageCache cache;
  const bool jacobi;
  // with the default runner the state stays in HBM (dpe_state_save / dpe_pm_stage_resident): the
  // prior, the source depths and the epilogue are all on the device, nothing is copied back per pass
  bool resident = false;
  Runner runner;
  std::unique_ptr<VizWriter> viz;   // declared after `runner`: joined before the context goes
  std::unique_ptr<PointCloudWriter> points;   // (the same)
  std::map<int, ColorImage> colour;      // point_cloud: the colour images of this rank's references, decoded once
  int w0 = 0, h0 = 0;               // the full image size (CheckImages: all the same)
  int round_num = 0, iteration_index = 0;
  std::map<int, ImageState> states;      // final states; with a runner hook also every pass's prior
  std::map<int, DepthMap> depth_cur;     // runner hook: the current depth map of every image of the run
  std::map<int, ImageState> fusion_states;   // what RunFusion reads: this rank's states and the gathered ones
  NativeFusion nf;                           // the device side of fusion and of the consistency maps

  Problem& problem_of(int rank, size_t k) { return problems[ranks.block(rank)[k]]; }
  // one rank has nobody to wait for: its first failure ends the run
  bool single_rank_failed() {
    if (ranks.multi() || !ranks.failed()) return false;
    err = ranks.first_error();
    return true;
  }
  bool images_error(const std::string& detail) {
    err = "Images may error, check it! " + detail;
    std::cerr << "Images may error, check it!\n";
    return false;
  }

  bool load_problems() {
    std::error_code ec;
    fs::create_directories(fs::path(dense) / kOutName, ec);
    return generate_sample_list(dense, problems, err);
  }

  // every image of the run decoded once, on the host threads; CheckImages (main.cpp:310-329); the split
  bool decode_and_check_images() {
    std::vector<int> ids;
    for (const Problem& p : problems) {
      ids.push_back(p.ref_image_id);
      for (int s : p.src_image_ids) ids.push_back(s);
    }
    std::string perr;
    if (!cache.prefetch(ids, perr)) return images_error(perr);
    bool ok = !problems.empty();
    for (size_t i = 0; ok && i < problems.size(); ++i) {
      int w, h;
      if (!cache.full(problems[i].ref_image_id, w, h, err)) ok = false;
      else if (i == 0) { w0 = w; h0 = h; }
      else if (w != w0 || h != h0) ok = false;
    }
    if (!ok) return images_error(err);
    const int n = (int)problems.size();
    // every rank reads the same pair.txt, so every rank takes this exit together (no collective yet)
    if (ranks.world() > n) {
      err = "world_size " + std::to_string(ranks.world()) + " exceeds the " + std::to_string(n) + " problems";
      return false;
    }
    ranks.split(n);
    return true;
  }

  bool open_runner() {
    if (opt.runner) { runner.fn = opt.runner; runner.user = opt.runner_user; return true; }
    runner.ctx = dpe_create(opt.gpu_index);
    if (!runner.ctx) ranks.fail(std::string("dpe_create: ") + dpe_last_error());
    else { runner.fn = native_runner; runner.user = runner.ctx; resident = true; }
    return !single_rank_failed();
  }

  void compute_round_num() {   // ComputeRoundNum (main.cpp:390-408)
    int max_size = std::max(w0, h0);
    round_num = 1;
    while (max_size > 800) { max_size /= 2; round_num++; }
    round_num = std::max(round_num, 2);
    for (auto& p : problems) p.params.max_scale_size = std::max(1, (int)std::pow(2, round_num - 1));
    if (opt.verbose && ranks.rank() == 0) {
      // std::cout as main.cpp:489, 504 (the pybind module redirects it into sys.stdout)
      std::cout << "There are " << problems.size() << " images to be processed!" << std::endl;
      std::cout << "There are " << round_num << " resolution stages for coarse-to-fine processing!" << std::endl;
      std::cout << "Iteration nums: " << round_num * 4 << std::endl;
    }
  }

  // GetProblemEdges for every scale of the schedule (main.cpp:494-501); images are independent,
  // so a pool of host threads takes them round-robin (the decode cache is filled first)
  bool edge_prepass() {
    const std::vector<int>& mine = ranks.mine();
    roctxRangePushA("GetProblemEdges");
    std::vector<GrayImage> grey(mine.size());
    for (size_t k = 0; k < mine.size(); ++k) {
      int fw, fh;
      const std::vector<float>* f = cache.full(problems[mine[k]].ref_image_id, fw, fh, err);
      if (!f) return false;   // decoded in CheckImages above: cannot fail here
      grey[k].w = fw; grey[k].h = fh;
      grey[k].px.resize(f->size());
      for (size_t q = 0; q < f->size(); ++q) grey[k].px[q] = (uint8_t)(*f)[q];
    }
    const int nt = std::max(1, std::min<int>(host_threads(), (int)grey.size()));
    // the data-parallel stages (resize, Sobel / NMS, Roberts) on the runner's GPU, the scan-order and
    // RNG-order parts (hysteresis walk, Connect, HoughLinesP) on the host threads
    std::mutex edge_mu;
    EdgeDevice edev{runner.ctx, &edge_mu};
    std::vector<std::string> terr(nt);
    run_on_threads(nt, [&](int t) {
      for (size_t k = t; k < grey.size(); k += nt) {
        const Problem& p = problems[mine[k]];
        for (int i = 0; i < round_num && terr[t].empty(); ++i)
          if (!get_problem_edges(grey[k], (int)std::pow(2, round_num - 1 - i), p.result_folder, p.params.use_edge,
                                 p.params.use_label, p.params.high_res_img, terr[t], &edev, opt.viz) && terr[t].empty())
            terr[t] = "EdgeSegment failed";
      }
    });
    roctxRangePop();
    for (auto& e : terr) if (!e.empty()) { ranks.fail(e); break; }
    return !single_rank_failed();
  }

  // ExportDepthImagePointCloud's inputs (DPE.cpp:1702-1708) for the W x H state of problem `p`: the
  // camera and the colour image (decoded once per run) through RescaleImageAndCamera.  *px: the pixels.
  bool point_cloud_inputs(const Problem& p, int W, int H, DpeCamera& cam, std::vector<uint8_t>& scaled, const uint8_t** px,
                          std::string& perr) {
    if (!read_camera(cam_path(p.dense_folder, p.ref_image_id), cam, perr)) return false;
    auto it = colour.find(p.ref_image_id);
    if (it == colour.end()) {
      ColorImage img;
      if (!read_bgr(image_path(p.dense_folder, p.ref_image_id), img, perr)) return false;
      it = colour.emplace(p.ref_image_id, std::move(img)).first;
    }
    const ColorImage& img = it->second;
    if (img.w != W || img.h != H) { resize_bgr_and_camera(img, W, H, cam, scaled); *px = scaled.data(); }
    else *px = img.bgr.data();
    cam.width = W; cam.height = H;
    return true;
  }
  // main.cpp:456: after the last pass of a resolution round
  bool point_cloud_due(const Problem& p) const { return opt.point_cloud != 0 && (p.iteration + 1) % 4 == 0; }
  static std::string point_cloud_path(const Problem& p) {
    return (fs::path(p.result_folder) / ("point_" + std::to_string(p.iteration) + ".ply")).string();
  }

  // stage, execute and save in HBM; nothing comes back unless the intermediate maps are asked for
  bool run_resident_pass(const Problem& p, const PassInput& pi, std::string& perr) {
    int rc = dpe_pm_stage_resident(runner.ctx, &pi.in, p.ref_image_id);
    if (rc == 0) rc = dpe_pm_execute(runner.ctx, nullptr);
    if (rc == 0) rc = dpe_state_save(runner.ctx, p.ref_image_id);
    if (rc != 0) { perr = "PatchMatch pass failed (" + std::to_string(rc) + "): " + dpe_last_error(); return false; }
    if (opt.keep_intermediate) {
      ImageState s;
      if (!fetch_state(runner.ctx, p.ref_image_id, s, perr)) return false;
      if (!write_state_maps(p, s, perr)) return false;
    }
    if (viz)   // main.cpp:448-454, from the saved (post-epilogue) state; the stream orders the next pass after it
      for (int kind = 0; kind < 3; ++kind)
        if (!viz->submit(p.ref_image_id, kind, p.params.depth_min, p.params.depth_max, pi.W, pi.H, viz_path(p, kind), perr))
          return false;
    if (point_cloud_due(p)) {   // main.cpp:456-466, from the saved state as well
      DpeCamera cam;
      std::vector<uint8_t> scaled;
      const uint8_t* px = nullptr;
      if (!point_cloud_inputs(p, pi.W, pi.H, cam, scaled, &px, perr)) return false;
      if (!points->submit(p.ref_image_id, opt.point_cloud, cam, px, p.params.depth_min, p.params.depth_max,
                          point_cloud_path(p), perr))
        return false;
    }
    return true;
  }

  // a runner hook keeps the state on the host: source depths and the prior rescaled here, the
  // runner, then ProcessProblem's epilogue into `states`
  bool run_hook_pass(const Problem& p, PassInput& pi, const std::map<int, DepthMap>& depth_src, std::string& perr) {
    const DpePatchMatchParams& P = p.params;
    const int W = pi.W, H = pi.H;
    const size_t L = (size_t)W * H;
    std::vector<std::vector<float>> dep_store;
    std::vector<const float*> depths(pi.ids.size(), nullptr);
    if (P.geom_consistency) {
      dep_store.reserve(pi.ids.size());
      for (size_t k = 1; k < pi.ids.size(); ++k) {
        auto it = depth_src.find(pi.ids[k]);
        if (it == depth_src.end()) { perr = "no depth map of source image " + std::to_string(pi.ids[k]); return false; }
        dep_store.push_back(rescaled(it->second.d, it->second.w, it->second.h, W, H));
        depths[k] = dep_store.back().data();
      }
      pi.in.depths = depths.data();
    }
    const ImageState* prev = states.count(p.ref_image_id) ? &states.at(p.ref_image_id) : nullptr;
    std::vector<float> planes(L * 4, 0.0f);
    std::vector<uint8_t> weak(L, DPE_STRONG);
    std::vector<uint32_t> sel(L, 0u);
    if (P.use_APD) {
      if (!prev) { perr = "Can't find weak info of image " + std::to_string(p.ref_image_id); return false; }
      weak = rescaled(prev->weak, prev->w, prev->h, W, H);
    }
    if (P.state != DPE_FIRST_INIT) {
      if (!prev) { perr = "no prior depth/normal of image " + std::to_string(p.ref_image_id); return false; }
      const std::vector<float> d = rescaled(prev->depth, prev->w, prev->h, W, H);
      const std::vector<float> n = rescaled(prev->normal, prev->w, prev->h, W, H, 3);
      for (size_t i = 0; i < L; ++i) {
        planes[4 * i + 0] = n[3 * i + 0]; planes[4 * i + 1] = n[3 * i + 1]; planes[4 * i + 2] = n[3 * i + 2];
        planes[4 * i + 3] = d[i];
      }
      sel = rescaled(prev->sel, prev->w, prev->h, W, H);
    }
    std::vector<float> costs(L);
    DpePassState st{planes.data(), weak.data(), sel.data(), costs.data()};
    const int rc = runner.fn(runner.user, &pi.in, &st);
    if (rc != 0) { perr = "PatchMatch pass failed (" + std::to_string(rc) + "): runner"; return false; }
    // epilogue (main.cpp:423-437): depth outside [dmin, dmax] -> 0 and UNKNOWN
    ImageState s;
    s.w = W; s.h = H;
    s.depth.resize(L); s.normal.resize(L * 3); s.weak = weak; s.sel = sel;
    for (size_t i = 0; i < L; ++i) {
      float d = planes[4 * i + 3];
      if (d < P.depth_min || d > P.depth_max) { d = 0.0f; s.weak[i] = DPE_UNKNOWN; }
      s.depth[i] = d;
      s.normal[3 * i + 0] = planes[4 * i + 0]; s.normal[3 * i + 1] = planes[4 * i + 1]; s.normal[3 * i + 2] = planes[4 * i + 2];
    }
    if (opt.keep_intermediate && !write_state_maps(p, s, perr)) return false;
    if (opt.viz) {   // main.cpp:448-454 on the host
      std::vector<uint8_t> bgr(L * 3);
      for (int kind = 0; kind < 3; ++kind) {
        viz_render(kind, W, H, s.depth.data(), s.normal.data(), s.weak.data(), P.depth_min, P.depth_max, bgr.data());
        if (!write_jpeg(viz_path(p, kind), bgr.data(), W, H, 3, kVizQuality, perr)) return false;
      }
    }
    if (point_cloud_due(p)) {   // main.cpp:456-466 on the host
      DpeCamera cam;
      std::vector<uint8_t> scaled;
      const uint8_t* px = nullptr;
      if (!point_cloud_inputs(p, W, H, cam, scaled, &px, perr)) return false;
      std::vector<FusedPoint> cloud(L);
      const long long n = depth_point_cloud(opt.point_cloud, W, H, s.depth.data(), s.weak.data(), cam, px, P.depth_min,
                                            P.depth_max, cloud.data(), cloud.size());
      if (n < 0) { perr = "point cloud failed"; return false; }
      if (!export_point_cloud(point_cloud_path(p), cloud.data(), (size_t)n, perr)) return false;
    }
    states[p.ref_image_id] = std::move(s);
    return true;
  }

  // pass j of round i over this rank's images; the first failure raises the flag and ends the block
  void run_block(int i, int j, int scale) {
    // runner hook, jacobi: every image of the block reads the depths of the previous pass round
    const std::map<int, DepthMap> snapshot = (jacobi && !resident) ? depth_cur : std::map<int, DepthMap>{};
    const auto& depth_src = jacobi ? snapshot : depth_cur;
    for (int pi : ranks.mine()) {
      if (ranks.failed()) break;
      Problem& p = problems[pi];
      p.iteration = iteration_index;
      p.scale_size = scale;
      p.params.scale_size = p.scale_size;
      pass_params(p.params, i, j);
      if (opt.max_iterations > 0) p.params.max_iterations = opt.max_iterations;
      if (opt.photometric_only) p.params.geom_consistency = false;
      std::string perr;
      const std::string rname = "ProcessProblem round " + std::to_string(i) + " pass " + std::to_string(j + 1) +
                                " image " + std::to_string(p.ref_image_id);
      roctxRangePushA(rname.c_str());
      PassInput in;
      const bool ok = build_pass_input(p, cache, opt.base_seed, in, perr) &&
                      (resident ? run_resident_pass(p, in, perr) : run_hook_pass(p, in, depth_src, perr));
      roctxRangePop();
      if (!ok) { ranks.fail(perr); break; }
      if (!resident) {
        const ImageState& s = states[p.ref_image_id];
        depth_cur[p.ref_image_id] = DepthMap{s.w, s.h, s.depth};
      }
    }
  }

  // All-gather of the pw x ph depth maps from / into the HBM-resident states.  Two collectives, both
  // joined by every rank whatever happened locally:
  //  1. the ranks' status flags over the host hook.  A local error before it (the pass, the exchange
  //     buffers, the export) raises the flag and every rank returns 1 at this exchange;
  //  2. the depth maps (max_block maps per rank), device to device, or one device -> host -> device
  //     hop through the host hook.  An error after (1) is recorded and reported at the next
  //     exchange's (1) or at the final status exchange after the passes.
  bool exchange_depths_resident(int pw, int ph) {
    DpeContext* ctx = runner.ctx;
    const int world = ranks.world(), rank = ranks.rank();
    const size_t per = (size_t)pw * ph, cnt = ranks.max_block() * per;
    float* dsend = dpe_device_buffer(ctx, 0, cnt);
    float* drecv = dsend ? dpe_device_buffer(ctx, 1, cnt * world) : nullptr;
    const bool dev_ok = drecv != nullptr;
    if (!dev_ok) ranks.fail(dpe_last_error());
    for (size_t k = 0; dev_ok && !ranks.failed() && k < ranks.mine().size(); ++k)
      if (dpe_state_export_depth(ctx, problem_of(rank, k).ref_image_id, dsend + k * per, nullptr) != 0)
        ranks.fail(dpe_last_error());
    // the exports run on the context's stream; the collective reads dsend from another one
    if (dev_ok && !ranks.failed() && dpe_sync(ctx) != 0) ranks.fail(dpe_last_error());
    if (ranks.fault_at(RankGroup::kBeforeExchange)) ranks.fail("injected fault before the exchange");
    if (!ranks.status_exchange(err)) return false;
    if (ranks.has_device_hook()) {
      if (!ranks.gather_device(dsend, cnt, drecv, err)) return false;
    } else {   // host hook: one device -> host -> device hop of the packed maps
      std::vector<float> hs(cnt, 0.0f), hr(cnt * world, 0.0f);
      if (dpe_device_copy(ctx, hs.data(), dsend, cnt * sizeof(float), 1) != 0) ranks.fail(dpe_last_error());
      if (!ranks.gather(hs.data(), cnt, hr.data(), err)) return false;
      if (!ranks.failed() && dpe_device_copy(ctx, drecv, hr.data(), hr.size() * sizeof(float), 0) != 0)
        ranks.fail(dpe_last_error());
    }
    if (ranks.fault_at(RankGroup::kAfterExchange)) ranks.fail("injected fault after the exchange");
    for (int r = 0; r < world; ++r) {
      if (r == rank) continue;
      for (size_t k = 0; k < ranks.block(r).size(); ++k)
        if (!ranks.failed() && dpe_state_import_depth(ctx, problem_of(r, k).ref_image_id, pw, ph,
                                                      drecv + (size_t)r * cnt + k * per, nullptr) != 0)
          ranks.fail(dpe_last_error());
    }
    if (!ranks.failed() && dpe_sync(ctx) != 0) ranks.fail(dpe_last_error());   // imports done: the exchange's end
    return true;
  }

  // runner hook: all-gather of the depth maps (the pass's only cross-image data) into depth_cur
  bool exchange_depths_host(int pw, int ph) {
    const size_t per = (size_t)pw * ph, nmax = ranks.max_block();
    std::vector<float> send(nmax * per, 0.0f), recv;
    for (size_t k = 0; !ranks.failed() && k < ranks.mine().size(); ++k)
      std::memcpy(send.data() + k * per, depth_cur[problem_of(ranks.rank(), k).ref_image_id].d.data(), per * 4);
    if (!ranks.exchange(send, recv, err)) return false;
    for (int r = 0; r < ranks.world(); ++r)
      for (size_t k = 0; k < ranks.block(r).size(); ++k) {
        const float* src = recv.data() + ((size_t)r * nmax + k) * per;
        depth_cur[problem_of(r, k).ref_image_id] = DepthMap{pw, ph, std::vector<float>(src, src + per)};
      }
    return true;
  }

  bool run_pass_round(int i, int j) {
    const double tp0 = now_s();
    if (resident && jacobi && !ranks.failed() && dpe_state_snapshot(runner.ctx) != 0) ranks.fail(dpe_last_error());
    // pass size: ImageCache::level's rounding of the first image (CheckImages: all the same size)
    const int scale = (int)std::pow(2, round_num - 1 - i);
    const int pw = scale == 1 ? w0 : std_round(w0 * (1.0f / (float)scale));
    const int ph = scale == 1 ? h0 : std_round(h0 * (1.0f / (float)scale));
    run_block(i, j, scale);
    // the pass round's GPU work is finished before its clock stops (and, multi-rank, before the
    // exchange's clock starts): with one rank the passes are otherwise only enqueued here
    if (resident && !ranks.failed() && dpe_sync(runner.ctx) != 0) ranks.fail(dpe_last_error());
    if (single_rank_failed()) return false;
    const double tx0 = now_s();
    g_times[kTimePassWork] += tx0 - tp0;
    if (ranks.multi()) {
      if (!(resident ? exchange_depths_resident(pw, ph) : exchange_depths_host(pw, ph))) return false;
      g_times[kTimeExchange] += now_s() - tx0;
    }
    if (opt.verbose && ranks.rank() == 0)
      std::cout << "Iteration " << iteration_index + 1 << " / " << round_num * 4 << " done" << std::endl;
    iteration_index++;
    return true;
  }

  void finish_viz() {   // the pictures still being coded or written; their errors
    std::string verr;
    if (viz && !viz->finish(verr)) ranks.fail(verr);
  }
  void finish_points() {   // the point clouds still being copied or written; their errors
    std::string perr;
    if (points && !points->finish(perr)) ranks.fail(perr);
  }

  void collect_final_states() {   // the final states come back from HBM once
    if (!resident || ranks.failed()) return;
    for (int pi : ranks.mine()) {
      std::string ferr;
      const int id = problems[pi].ref_image_id;
      if (!fetch_state(runner.ctx, id, states[id], ferr)) { ranks.fail(ferr); break; }
    }
  }

  void write_all_outputs() {   // each image's .npy files on their own host thread (independent files)
    if (ranks.failed()) return;
    const std::vector<int>& mine = ranks.mine();
    const int nt = std::max(1, std::min<int>(host_threads(), (int)mine.size()));
    std::vector<std::string> werr(mine.size());
    run_on_threads(nt, [&](int t) {
      for (size_t k = t; k < mine.size(); k += nt) {
        const Problem& p = problems[mine[k]];
        if (!write_outputs(p, states.at(p.ref_image_id), opt, werr[k]) && werr[k].empty()) werr[k] = "write failed";
      }
    });
    for (auto& e : werr) if (!e.empty()) { ranks.fail(e); break; }
  }

  // fusion_states: this rank's final states and, with several ranks, every other image's depth (the
  // last exchange left it here), normals and pixel states (one more exchange)
  bool gather_states_for_fusion() {
    for (int pi : ranks.mine()) fusion_states[problems[pi].ref_image_id] = states[problems[pi].ref_image_id];
    if (!ranks.multi()) return true;
    const ImageState& s0 = states[problem_of(ranks.rank(), 0).ref_image_id];
    const size_t per = (size_t)s0.w * s0.h, nmax = ranks.max_block();
    std::vector<float> send(nmax * per * 4, 0.0f), recv;
    for (size_t k = 0; k < ranks.mine().size(); ++k) {
      const ImageState& st = states[problem_of(ranks.rank(), k).ref_image_id];
      float* o = send.data() + k * per * 4;
      std::memcpy(o, st.normal.data(), per * 12);
      for (size_t i = 0; i < per; ++i) o[3 * per + i] = (float)st.weak[i];
    }
    if (!ranks.exchange(send, recv, err)) return false;
    for (int r = 0; r < ranks.world(); ++r)
      for (size_t k = 0; k < ranks.block(r).size(); ++k) {
        const int id = problem_of(r, k).ref_image_id;
        if (fusion_states.count(id)) continue;
        const float* src = recv.data() + ((size_t)r * nmax + k) * per * 4;
        ImageState st;
        st.w = s0.w; st.h = s0.h;
        if (resident) {
          ImageState d;
          if (!fetch_state(runner.ctx, id, d, err, true)) return false;
          st.depth = std::move(d.depth);
        } else {
          st.depth = depth_cur[id].d;
        }
        st.normal.assign(src, src + 3 * per);
        st.weak.resize(per);
        for (size_t i = 0; i < per; ++i) st.weak[i] = (uint8_t)src[3 * per + i];
        fusion_states[id] = std::move(st);
      }
    return true;
  }

  // each view on its own host thread (independent files, independent outputs)
  bool load_fusion_views(std::vector<FusionView>& views) {
    const size_t nv = problems.size();
    views.resize(nv);
    const bool use_block = fs::exists(fs::path(dense) / "blocks");
    std::vector<std::string> verr(nv);
    const int nt = std::max(1, std::min<int>(host_threads(), (int)nv));
    run_on_threads(nt, [&](int t) {
      for (size_t i = t; i < nv; i += nt)
        if (!load_fusion_view(problems[i], fusion_states.at(problems[i].ref_image_id), use_block, views[i], verr[i]) &&
            verr[i].empty())
          verr[i] = "fusion view load failed";
    });
    for (auto& e : verr) if (!e.empty()) { err = e; return false; }
    return true;
  }

  // the context of the device fusion and the device consistency maps: the runner's, or (runner hook) one of its own
  bool open_fusion_context() {
    if (nf.ctx) return true;
    nf.ctx = runner.ctx;
    if (!nf.ctx) {
      nf.ctx = dpe_create(opt.gpu_index);
      if (!nf.ctx) { err = std::string("dpe_create: ") + dpe_last_error(); return false; }
      nf.own = true;
    }
    return true;
  }

  // consistency.npy / depth_filtered.npy of this rank's images against the gathered final states.  The
  // problems as indices into the views by FusionPlan (host.h).  fusion_runner == NULL: every image on the device, the views staged once (and left for
  // ETH3D fusion); else dpe_host_consistency's loop on host threads, one image each.
  bool write_consistency_maps() {
    const int n = (int)problems.size();
    std::vector<DpeFusionView> cv(n);
    std::vector<FusionPlan::Image> images;
    for (int i = 0; i < n; ++i) {
      const Problem& p = problems[i];
      if (!map_view(p, fusion_states.at(p.ref_image_id), w0, h0, cv[i], err)) return false;
      images.emplace_back(p.ref_image_id, &p.src_image_ids);
    }
    const std::vector<int>& mine = ranks.mine();
    const FusionPlan plan(images, &mine);
    const std::vector<int>& refs = plan.refs;
    const std::vector<std::vector<int>>& srcs = plan.srcs;
    for (size_t k = 0; k < mine.size(); ++k) {
      const Problem& p = problems[mine[k]];
      std::string aerr;
      if (!consistency_args_ok(n, refs[k], srcs[k].data(), (int)srcs[k].size(), opt.consistency, aerr)) {
        err = aerr + " (image " + std::to_string(p.ref_image_id) + ")";
        return false;
      }
    }
    auto write_maps = [&](size_t k, const uint8_t* count, const float* filtered, std::string& werr) {
      const DpeFusionView& R = cv[refs[k]];
      const fs::path rf(problems[mine[k]].result_folder);
      const std::vector<int64_t> hw{R.height, R.width};
      return write_npy((rf / "consistency.npy").string(), count, hw, "|u1", 1, werr) &&
             write_npy((rf / "depth_filtered.npy").string(), filtered, hw, "<f4", 4, werr);
    };
    if (opt.fusion_runner) {
      const int nt = std::max(1, std::min<int>(host_threads(), (int)mine.size()));
      std::vector<std::string> terr(mine.size());
      run_on_threads(nt, [&](int t) {
        for (size_t k = t; k < mine.size(); k += nt) {
          const size_t L = (size_t)cv[refs[k]].width * cv[refs[k]].height;
          std::vector<uint8_t> count(L);
          std::vector<float> filtered(L);
          consistency_image(cv.data(), refs[k], srcs[k].data(), (int)srcs[k].size(), opt.consistency, count.data(),
                            filtered.data());
          if (!write_maps(k, count.data(), filtered.data(), terr[k]) && terr[k].empty()) terr[k] = "write failed";
        }
      });
      for (auto& e : terr) if (!e.empty()) { err = e; return false; }
      return true;
    }
    float D = 0.0f;
    if (!consistency_dot_threshold(D, err)) return false;
    if (!open_fusion_context()) return false;
    if (nf.stage(cv.data(), n) != DPE_OK) { err = "dpe_fusion_stage: " + nf.err; return false; }
    std::vector<uint8_t> count;
    std::vector<float> filtered;
    for (size_t k = 0; k < mine.size(); ++k) {
      const size_t L = (size_t)cv[refs[k]].width * cv[refs[k]].height;
      count.resize(L); filtered.resize(L);
      if (dpe_fusion_consistency(nf.ctx, refs[k], srcs[k].data(), (int)srcs[k].size(), D, opt.consistency, count.data(),
                                 filtered.data()) != DPE_OK) {
        err = std::string("dpe_fusion_consistency: ") + dpe_last_error();
        return false;
      }
      if (!write_maps(k, count.data(), filtered.data(), err)) return false;
    }
    return true;
  }

  bool fuse_and_export(std::vector<FusionView>& views) {   // RunFusion + ExportPointCloud (main.cpp:578-580)
    dpe_fusion_fn ffn = opt.fusion_runner;
    void* fuser = opt.fusion_user;
    if (!ffn) {
      if (!open_fusion_context()) return false;
      ffn = native_fusion; fuser = &nf;
    }
    std::vector<FusedPoint> cloud;
    if (opt.fusion_mode != DPE_FUSION_ETH3D) {   // the Tanks-and-Temples variants: on the device, or (hook) serial
      if (!run_fusion_tat(views, opt.fusion_mode, opt.fusion_runner ? nullptr : nf.ctx, cloud, err)) return false;
    } else if (!run_fusion(views, ffn, fuser, cloud, err)) {
      if (!opt.fusion_runner) err += std::string(": ") + (nf.err.empty() ? std::string(dpe_last_error()) : nf.err);
      return false;
    }
    if (!export_point_cloud((fs::path(dense) / kOutName / "DPE.ply").string(), cloud, err)) return false;
    if (opt.verbose) std::cout << "Fused " << cloud.size() << " points" << std::endl;
    return true;
  }

  void remove_intermediate_maps() {   // the reference's clean-up (main.cpp:581-595)
    for (int pi : ranks.mine())
      for (int j = 0; j < round_num; j++) {
        std::error_code ec;
        fs::remove(fs::path(problems[pi].result_folder) / ("edges_" + std::to_string(j) + ".dmb"), ec);
        fs::remove(fs::path(problems[pi].result_folder) / ("labels_" + std::to_string(j) + ".dmb"), ec);
      }
  }
};

int run(const char* dense_folder, const DpePipelineOptions& opt) {
  std::string& err = g_err;
  err.clear();
  const double t_start = now_s();
  for (double& t : g_times) t = 0.0;
  if (opt.world_size > 1 && !opt.allgather) { err = "world_size > 1 needs an all-gather"; return 1; }
  if (opt.rank < 0 || opt.rank >= std::max(1, opt.world_size)) { err = "bad rank"; return 1; }
  if (opt.fusion_mode != DPE_FUSION_ETH3D && opt.fusion_mode != DPE_FUSION_TAT_INTERMEDIATE &&
      opt.fusion_mode != DPE_FUSION_TAT_ADVANCED) {
    err = "bad fusion_mode " + std::to_string(opt.fusion_mode) + " (0 = ETH3D, 1 = TAT intermediate, 2 = TAT advanced)";
    return 1;
  }
  if (opt.point_cloud != 0 && opt.point_cloud != DPE_POINTS_ALL && opt.point_cloud != DPE_POINTS_STRONG) {
    err = "bad point_cloud " + std::to_string(opt.point_cloud) + " (0 = off, 1 = all pixels, 2 = STRONG pixels only)";
    return 1;
  }
  if (opt.consistency < 0 || opt.consistency > 255) {
    err = "bad consistency " + std::to_string(opt.consistency) + " (0 = off, 1..255 = min_views)";
    return 1;
  }
  PipelineRun r(dense_folder, opt, err);
  RankGroup& ranks = r.ranks;
  if (!r.load_problems()) return 1;
  double t_mark = now_s();
  auto lap = [&t_mark](TimeSlot slot) { const double t = now_s(); g_times[slot] = t - t_mark; t_mark = t; };
  if (!r.decode_and_check_images()) return 1;
  if (!r.open_runner()) return 1;
  r.compute_round_num();
  lap(kTimeDecode);
  if (!r.edge_prepass()) return 1;
  lap(kTimeEdges);
  if (opt.viz && r.resident) r.viz.reset(new VizWriter(r.runner.ctx, r.w0, r.h0));
  if (opt.point_cloud != 0 && r.resident) r.points.reset(new PointCloudWriter(r.runner.ctx, r.w0, r.h0));
  for (int i = 0; i < r.round_num; ++i)
    for (int j = -1; j < 3; ++j)
      if (!r.run_pass_round(i, j)) return 1;
  lap(kTimePasses);
  r.finish_viz();
  r.finish_points();
  r.collect_final_states();
  r.write_all_outputs();
  // every rank learns here whether any rank failed after its last exchange (a rank returning alone
  // would leave the others' next collective, or their success, inconsistent with it)
  if (ranks.multi() && !ranks.status_exchange(err)) return 1;
  if (ranks.failed()) { err = ranks.first_error(); return 1; }
  if (opt.fusion || opt.consistency) {   // both read every rank's final states (a collective: the options are the run's)
    const double t_gather0 = now_s();
    if (!r.gather_states_for_fusion()) return 1;
    g_times[opt.fusion ? kTimeFusion : kTimeConsistency] = now_s() - t_gather0;
  }
  if (opt.consistency) {   // every rank, its own images; before fusion, which finds the views staged
    const double t_cons0 = now_s();
    if (!r.write_consistency_maps()) return 1;
    g_times[kTimeConsistency] += now_s() - t_cons0;
  }
  if (opt.fusion) {   // RunFusion (main.cpp:578-580) on rank 0, over every rank's final states
    const double t_fusion0 = now_s();
    std::vector<FusionView> views;
    if (ranks.rank() == 0 && !(r.load_fusion_views(views) && r.fuse_and_export(views))) return 1;
    g_times[kTimeFusion] += now_s() - t_fusion0;
  }
  if (!opt.keep_intermediate) r.remove_intermediate_maps();
  if (opt.verbose && ranks.rank() == 0) std::cout << "All done" << std::endl;
  g_times[kTimeOutputs] = now_s() - t_mark;
  g_times[kTimeTotal] = now_s() - t_start;
  return 0;
}

}  // namespace
}  // namespace dpe_host

namespace dpe_host {
void set_last_error(const std::string& msg) { g_err = msg; }
}  // namespace dpe_host

extern "C" {

void dpe_pipeline_default_options(DpePipelineOptions* o) {
  std::memset(o, 0, sizeof(*o));
  o->gpu_index = 0;
  o->verbose = true; o->fusion = false; o->viz = false;
  o->depth = true; o->normal = false; o->weak = false; o->edge = false;
  o->schedule = DPE_SCHEDULE_REFERENCE;
  o->rank = 0; o->world_size = 1;
  o->base_seed = 0x5EED;
}

int dpe_run_pipeline(const char* dense_folder, const DpePipelineOptions* opt) {
  DpePipelineOptions o;
  if (opt) o = *opt; else dpe_pipeline_default_options(&o);
  try {
    return dpe_host::run(dense_folder, o);
  } catch (const std::exception& e) {
    dpe_host::g_err = e.what();
    return 1;
  }
}

const char* dpe_pipeline_last_error(void) { return dpe_host::g_err.c_str(); }

int dpe_pipeline_last_timings(double* out, int n) {
  int k = 0;
  for (; k < n && k < dpe_host::kNumTimes; ++k) out[k] = dpe_host::g_times[k];
  return k;
}

}  // extern "C"
