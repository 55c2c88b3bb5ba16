// dpe_context.h -- what a DpeContext (include/dpe_mvs.h) holds: device arrays, streams and events that
// own their HIP resources, the cached images, the resident states and the context itself, its members
// grouped by the unit that owns them.  Internal to the library and shared by its units (dpe_mvs.hip,
// dpe_state.hip, dpe_edges.hip, dpe_viz.hip, dpe_fusion.hip, dpe_points.hip, dpe_cloud.hip): every type here is an ordinary named
// type and the byte counter has one definition in the process.  Includes no kernel header.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "pass_common.h"
#include "tap_launch.h"          // ImgClass
#include "dpe_fusion_types.h"
#include "cloud_dist.h"          // CloudGrid

namespace dpe {

inline std::atomic<long long> g_live_bytes{0};   // dpe_live_device_bytes: what every DevArr of the process holds

// A device array that owns its allocation (move-only; freed with its owner).  ensure() only grows,
// and keeps 256 bytes behind the last element.
template <class T>
struct DevArr {
  T* p = nullptr;
  size_t n = 0;
  DevArr() = default;
  DevArr(DevArr&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DevArr& operator=(DevArr&& o) noexcept { std::swap(p, o.p); std::swap(n, o.n); return *this; }
  DevArr(const DevArr&) = delete;
  DevArr& operator=(const DevArr&) = delete;
  ~DevArr() { reset(); }
  hipError_t ensure(size_t count) {
    if (count <= n && p) return hipSuccess;
    reset();
    hipError_t e = hipMalloc((void**)&p, count * sizeof(T) + 256);
    if (e != hipSuccess) { p = nullptr; return e; }
    n = count;
    g_live_bytes += (long long)bytes();
    return e;
  }
  size_t bytes() const { return p ? n * sizeof(T) + 256 : 0; }

 private:
  void reset() {
    if (p) { g_live_bytes -= (long long)bytes(); (void)hipFree(p); }
    p = nullptr; n = 0;
  }
};

// a stream / an event of the context: created after construction (create() returns the error),
// destroyed with its owner
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() { if (s) (void)hipStreamDestroy(s); }
  hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
  operator hipStream_t() const { return s; }
};
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() { if (e) (void)hipEventDestroy(e); }
  hipError_t create(unsigned flags = hipEventDisableTiming) { return hipEventCreateWithFlags(&e, flags); }
  operator hipEvent_t() const { return e; }
};

// An image kept in HBM across passes (DpePassInput.image_ids): its f32 grey levels and the gather
// layouts built from them.
struct CachedImage {
  int id = 0, W = 0, H = 0;
  int cls = IMG_F32;        // ImgClass of the grey levels
  DevArr<float> plain;
  DevArr<uint32_t> q8;      // TEX_U8 quad texels (8-bit images)
  DevArr<uint2> q16;        // TEX_F16 quad texels (8-bit images)
  DevArr<uint32_t> qp;      // TEX_P16 column pairs (8-bit images)
  DevArr<float4> qf;        // f32 quad texels (built on demand)
  uint64_t last_use = 0;
  size_t bytes() const { return plain.n * 4 + q8.n * 4 + q16.n * 8 + qp.n * 4 + qf.n * 16; }
};

// Per-image pipeline state kept in HBM between passes (the reference's depths.dmb / normals.dmb /
// weak.bin / selected_views.bin round trip, main.cpp:439-446 -> DPE.cpp:826-911).  dpe_state.hip.
struct ResState {
  int w = 0, h = 0;
  bool full = false;          // planes / weak / sel of a pass of this image; false: depth only (imported)
  DevArr<float4> planes;      // (world normal xyz, depth) after the ProcessProblem epilogue
  DevArr<uint8_t> weak;
  DevArr<uint32_t> sel;
  DevArr<float> snap;         // depth snapshot for the Jacobi schedule (dpe_state_snapshot)
  int snap_w = 0, snap_h = 0;
  bool has_snap = false;
};

// What the pass works in (dpe_mvs.hip: dpe_pm_stage / dpe_pm_execute): its settings and records, the
// staged inputs, the initial state, the working set and the pixel lists.
struct PassWork {
  bool staged = false;
#if DPE_GN_ONCE
  bool gn_done_for_stage = false;    // GenNeighbours' outputs of this staged state are kept
  DevArr<float> gn_complex;          //   and complex_ after GenNeighbours
#endif
  bool timing = false;
  bool counting = false;
  int gn_slots = 0;                  // DPE_OPT_GN_SLOTS (0 = by rotate_time)
  float timings[DPE_NUM_CLASSES + 1] = {0};
  int launches[DPE_NUM_CLASSES + 1] = {0};
  unsigned long long counts[DPE_NUM_CLASSES * 4] = {0};
  DevArr<unsigned long long> cnt;
  DevArr<unsigned long long> phase;  // DPE_PHASE_PROF builds: per-phase cycle sums
  PassConst hc;                      // host copy of the pass constants
  DevArr<PassConst> dc;
  // inputs
  DevArr<float> img_plain[DPE_MAX_IMAGES];  // plain f32 images (ref used directly)
  DevArr<float4> imgq[DPE_MAX_IMAGES];
  DevArr<uint32_t> imgq8_all;        // all 8-bit quad images, TEX_U8 layout, one allocation
  DevArr<uint2> imgq16_all;          //   and TEX_F16 layout (32-bit tap offsets)
  DevArr<uint32_t> imgqp_all;        //   and TEX_P16 column pairs
  int img_cls = IMG_F32;             // ImgClass of the pass (the narrowest class of its views)
  DevArr<float> depth[DPE_MAX_IMAGES];
  DevArr<uint8_t> edge, edge_low;
  DevArr<int> label;
  // staged initial state
  DevArr<float4> planes0;
  DevArr<uint8_t> weak0;
  DevArr<uint32_t> sel0;
  // working state
  DevArr<float4> planes, planes_snap, fit_plane;
  DevArr<float> costs, costs_snap, complex_;
  DevArr<uint32_t> sel, sel_snap;
  DevArr<uint8_t> weak, weak_rel, vw;
  DevArr<short2> nb, nearest, edge_neigh, lab_bound;
  DevArr<int> radius;
  DevArr<int> tab_right, tab_down;   // FindNearestStrongPoint tables
  DevArr<int> gn_ovf;                // GenNeighbours pixels left to the scratch kernel (k_gen_neighbours_lds)
  DevArr<float> gn_tab;              // normalised image coordinates per column / row (k_gn_tables)
  // the pass's pixel lists; their regions are named by PassLists (pass_lists.h)
  DevArr<int> lists, row_counts, list_totals;   // pixel indices / per-row counts / one total per list
  DevArr<int> part_cnt;                          // per colour: chunk counts / offsets of the weak-list partition
  DevBufs bufs;
};

// EdgeSegment stages (dpe_edges.hip: dpe_canny / dpe_resize_* / dpe_roberts_threshold): scratch
struct EdgeScratch {
  DevArr<uint8_t> a, b, map;
  DevArr<float> fa, fb;
  DevArr<int> rows, mag, itab;
  DevArr<int16_t> dx, dy;
  DevArr<float> ftab;
  DevArr<short> stab;
};

// the views of a fusion (dpe_fusion.hip: dpe_fusion_stage / dpe_fusion_candidates / dpe_fusion_consistency)
struct FusionStage {
  std::vector<DevArr<float>> depth, normal;
  std::vector<FusionViewDev> host;
  DevArr<FusionViewDev> views;
  DevArr<DpeCamera> cams;
  DevArr<int> src;
  DevArr<int32_t> idx;
  DevArr<float> val;
  DevArr<uint8_t> cons_count;        // dpe_fusion_consistency: the reference view's consistency count
  DevArr<float> cons_depth;          //   and its filtered depth map
  int n = 0;
};

// the Tanks-and-Temples fusions (dpe_fusion.hip: dpe_fusion_tat_begin / dpe_fusion_tat_image), over the
// staged views.  `ev` is declared first and so outlives the buffers.
struct TatFusion {
  Event ev;                          // end of the last copy-out of dpe_fusion_tat_image (on the aux stream)
  std::vector<DevArr<uint8_t>> bgr, block, mask;
  DevArr<TatViewDev> views;
  bool ready = false;
  DevArr<float> dthr;                // dot-product thresholds of the angle test, by k
  DevArr<int> last, agg;             // per (view, pixel) last hit of the block / per (view, chunk) carry
  DevArr<int> cnt, tot;              // fused pixels per chunk -> offsets; the image's total
  DevArr<uint8_t> emit;
  DevArr<TatPoint> rec;              // per pixel: the point it contributes
  DevArr<TatPoint> out[2];           // compacted points, double-buffered: the copy-out of one image
  int turn = 0;                      //   runs on the aux stream beside the kernels of the next
  bool copying = false;              // `ev` recorded and not yet waited for
  // the colours and masks of dpe_fusion_tat_begin belong to the views staged before: a new
  // dpe_fusion_stage makes dpe_fusion_tat_image wait for a new dpe_fusion_tat_begin
  void views_restaged() { ready = false; }
};

// viz medium results (dpe_viz.hip: dpe_state_render*): scratch, allocated on first use.  `ev` is
// declared first and so outlives the buffers.
struct VizScratch {
  std::mutex mu;                     // guards ev (dpe_state_render_wait runs on other host threads)
  std::map<const void*, Event> ev;   // per host block buffer: end of the last copy into it
  DevArr<uint8_t> bgr;               // the rendered picture
  DevArr<int16_t> blocks;            // its quantised JPEG blocks
  DevArr<uint16_t> q;                // quantisation tables of `quality` (64 luma + 64 chroma)
  int quality = 0;
  DevArr<float4> planes;             // dpe_viz_render_arrays: the caller's arrays
  DevArr<uint8_t> weak;
};

// per-image point clouds (dpe_points.hip: dpe_state_point_cloud / dpe_point_cloud_arrays): scratch,
// allocated on first use.  `ev` is declared first and so outlives the buffers.
struct PointsScratch {
  std::mutex mu;                     // guards ev (dpe_state_point_cloud_wait runs on other host threads)
  std::map<const void*, Event> ev;   // per host point buffer: end of the last copy into it
  DevArr<uint8_t> bgr;               // the colour image at the map size
  DevArr<int> cnt, tot;              // valid pixels per (column, row segment) -> offsets; the image's total
  DevArr<TatPoint> out;              // the points in the reference's order
  DevArr<float4> planes;             // dpe_point_cloud_arrays: the caller's arrays
  DevArr<uint8_t> weak;
};

// The cloud section (dpe_cloud.hip): scratch, allocated on first use and grown on demand.
//
// its timer (dpe_set_timing): ev[0] is the start of the call, ev[k] its k-th mark, and slot[k - 1] the entry of ms[]
// that the time from ev[k - 1] to ev[k] is added to
struct CloudTimer {
  std::vector<Event> ev;             // the pool, grown on demand
  std::vector<int> slot;
  bool on = false;                   // the call in flight is timed
  float ms[4] = {0, 0, 0, 0};        // dpe_cloud_last_timings: the parts of the last call (include/dpe_mvs.h names them)
  bool timed = false;
};
// dpe_cloud_voxel (pass_voxel.h); the cloud is staged in pts[0], its bounds in bounds[0..7]
struct VoxelScratch {
  DevArr<uint8_t> rgb;               // the colours as the caller packs them, u8 [n][3]
  DevArr<int4> cell;                 // per point: cell and valid flag
  DevArr<uint32_t> frac;             // per point: the three lattice fractions
  DevArr<int> owner, count;          // the table, per slot
  DevArr<uint32_t> first;
  DevArr<unsigned long long> sum, csum;   // per slot and axis / channel
  DevArr<int> slot_at, bcnt;         // per point: the slot it is the first point of, or -1; per block: marked -> offsets
  DevArr<uint32_t> err;              // the insert kernel's error word
  DevArr<float> out_xyz;             // the records
  DevArr<uint8_t> out_rgb;
  DevArr<int> out_first, out_count;
};
// the ICP step (pass_register.h) over a staged pair: the source in pts[0], the target in pts[1], the target's grid
// in st / tcnt
struct IcpStage {
  DevArr<float> moved;               // the source under the step's transform, f32 [n][3]
  DevArr<double> part[2];            // the sums' partials, 16 per block, level by level
  DevArr<unsigned long long> matched;
  size_t n = 0, m = 0, tfinite = 0;
  CloudGrid grid;
  double os[3] = {0, 0, 0}, ot[3] = {0, 0, 0};   // per-axis minima of the finite source / target points
};
// the depth-map evaluation (pass_render.h): a staged scan is pts[0]; the rendered map is its own
struct RenderStage {
  size_t n = 0;
  DevArr<uint32_t> map;              // the z-buffer of the last view, after k_render_finish the map f32 [h][w]
  int map_w = 0, map_h = 0;          // 0: no map rendered yet
};
// dpe_depth_score and dpe_normal_score (score_run): every call uploads or zeroes what it reads here, so nothing in
// these buffers is resident between calls and the two scores share them.  The resident maps are render.map and
// normals.map
struct ScoreScratch {
  DevArr<float> est, gt, err;        // the caller's maps and the error map
  DevArr<double> part[2];            // the sums' partials, level by level
  DevArr<unsigned long long> cnt;    // n_gt, n_est, n_both, within[16], then the metric's bins
};
// the normal-map evaluation (pass_normals.h): the cloud of dpe_cloud_normals is pts[0] and its grid st / tcnt; a staged
// scan's normals sit beside pts[0]; a view with normals renders into `zb` first and leaves the depth map in render.map
struct NormalScratch {
  DevArr<float> normal;              // dpe_cloud_normals: the normals, f32 [n][3], by original index
  DevArr<int> count;                 //   the neighbour counts
  DevArr<long long> sums;            //   the ten sums per point, when asked for
  DevArr<float> staged;              // the staged scan's normals, f32 [n][3]
  bool has_staged = false;           // the staging in pts[0] came with normals
  DevArr<unsigned long long> zb;     // the z-buffer with winners: bits(z) << 32 | index
  DevArr<int> winner;                // per pixel the winning point, -1 where empty
  DevArr<float> map;                 // the rendered normal map, f32 [h][w][3]
  int map_w = 0, map_h = 0;          // 0: no normal map rendered yet
  DevArr<float> edges;               // dpe_normal_score: the 180 bin edges, uploaded once
};
// what stays in pts[] for later calls.  The calls that restage pts[] (nn, pair, index, voxel, normals, icp_stage,
// render_stage, render_stage_normals) end it; icp_step, render_view, render_view_normals, depth_score and normal_score
// leave it alone
enum class CloudResident { None, IcpPair, RenderScan };

// `timer` (its events) is declared first and so outlives the buffers.
struct CloudScratch {
  CloudTimer timer;
  // what is staged
  DevArr<float> pts[2];              // the two clouds as the caller packs them, f32 [k][3]
  DevArr<uint32_t> bounds;           // per cloud 8 words: k_cloud_bounds' keys and the finite count
  CloudResident resident = CloudResident::None;
  // the grid and the query (pass_cloud.h)
  DevArr<float4> st, sq;             // target / query points in bucket order: (x, y, z, original index)
  DevArr<int> tcnt, qcnt;            // per bucket: counts -> starts -> ends
  DevArr<float> out;                 // the distances, by original index
  DevArr<int> idx;                   // the matches, by original index (dpe_cloud_nn_index, the ICP step)
  VoxelScratch voxel;
  IcpStage icp;
  RenderStage render;
  ScoreScratch score;
  NormalScratch normals;
};

}  // namespace dpe

// Every member owns what it holds, so `delete ctx` frees the context.  Members are destroyed in
// reverse order: the streams and events are declared first and so outlive every buffer (the events of
// one group alone, tat.ev, viz.ev, points.ev and cloud.timer.ev, are the first members of their group).
struct DpeContext {
  int device = 0;
  dpe::Stream stream;
  dpe::Stream aux;                   // GenNeighbours beside the first strong half-sweep
  dpe::Event ev_fork, ev_join, ev_ei;
  dpe::Event ev_done;                // end of the last dpe_pm_execute's work on its stream
  dpe::Event ev_start;               // timing: start of the pass
  std::vector<dpe::Event> ev;        // timing: (start, end) per launch class slot
  bool pending = false;              // ev_done recorded and not yet waited for
  std::map<int, dpe::ResState> rstore;   // node addresses are stable: StageSrc points into it
  bool snap_mode = false;            // stage_resident reads source depths from the Jacobi snapshots
  dpe::DevArr<float> xbuf[2];        // dpe_device_buffer: exchange buffers of the multi-rank schedule
  std::vector<std::unique_ptr<dpe::CachedImage>> icache;
  uint64_t icache_clock = 0;
  dpe::PassWork pass;
  dpe::EdgeScratch edges;
  dpe::FusionStage fz;
  dpe::TatFusion tat;
  dpe::VizScratch viz;
  dpe::PointsScratch points;
  dpe::CloudScratch cloud;
};
