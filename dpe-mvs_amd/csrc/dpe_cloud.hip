// dpe_cloud.hip -- the cloud evaluation's distances (dpe_cloud_nn, dpe_cloud_nn_pair), the voxel
// down-sampling (dpe_cloud_voxel) and the registration's device half (dpe_cloud_nn_index, dpe_cloud_icp_stage,
// dpe_cloud_icp_step), the depth-map evaluation (dpe_cloud_render_stage, dpe_cloud_render_view, dpe_depth_score) and
// the normal-map evaluation (dpe_cloud_normals, dpe_cloud_render_stage_normals, dpe_cloud_render_view_normals,
// dpe_normal_score; one render_view and one score_run<Metric> serve both) of include/dpe_mvs.h: the kernels of
// pass_cloud.h, pass_voxel.h, pass_register.h, pass_render.h, pass_normals.h and tree_sum.h over the context's cloud
// scratch.  A unit of libdpe_mvs.so; the concurrency contract is dpe_mvs.hip's (dpe_entry.h): these calls wait until
// the context is quiet, use its stream and return with it synchronised.
//
// Every call opens with cloud_begin, launches through LAUNCH and, when it ran to its end, closes with timer_finish:
// a call that returns early (an empty cloud, nothing to match, an error) leaves no timings.
#include <hip/hip_runtime.h>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>

#include "pass_cloud.h"
#include "pass_voxel.h"
#include "pass_register.h"
#include "pass_render.h"
#include "pass_normals.h"
#include "dpe_entry.h"
#include "dpe_context.h"

using namespace dpe;

static_assert(kCloudBlock == kTreeBlock && kRenderBlock == kTreeBlock && kVoxelBlock == kTreeBlock && kNormalBlock == kTreeBlock,
              "every kernel of the section runs in blocks of the tree's 256 leaves");

static std::atomic<long long> g_cloud_launches{0};

extern "C" long long dpe_cloud_launches(void) { return g_cloud_launches.load(); }

// the one way this unit launches a kernel: on the context's stream, checked and counted
#define LAUNCH(kernel, blocks, c, ...)                                       \
  do {                                                                       \
    kernel<<<(blocks), kTreeBlock, 0, (c)->stream>>>(__VA_ARGS__);           \
    HIPC(hipGetLastError());                                                 \
    g_cloud_launches += 1;                                                   \
  } while (0)

namespace {

// what k_cloud_bounds found in one cloud
struct CloudBounds {
  float lo[3], hi[3];
  size_t finite;
};

float cloud_unkey(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  float f;
  memcpy(&f, &u, sizeof f);
  return f;
}

unsigned cloud_blocks(size_t n) { return (unsigned)((n + kTreeBlock - 1) / kTreeBlock); }

// the timer: an event of the pool recorded on the stream, the pool grown on demand
int timer_record(DpeContext* c, size_t k) {
  CloudTimer& t = c->cloud.timer;
  while (t.ev.size() <= k) {
    Event e;
    HIPC(e.create(hipEventDefault));
    t.ev.push_back(std::move(e));
  }
  HIPC(hipEventRecord(t.ev[k], c->stream));
  return DPE_OK;
}

// the end of a part of the call: its time since the mark before goes to ms[slot]
int timer_mark(DpeContext* c, int slot) {
  CloudTimer& t = c->cloud.timer;
  if (!t.on) return DPE_OK;
  t.slot.push_back(slot);
  return timer_record(c, t.slot.size());
}

// after the call's last mark: fills ms[]
int timer_finish(DpeContext* c) {
  CloudTimer& t = c->cloud.timer;
  if (!t.on) return DPE_OK;
  HIPC(hipEventSynchronize(t.ev[t.slot.size()]));
  for (float& ms : t.ms) ms = 0.f;
  for (size_t k = 0; k < t.slot.size(); ++k) {
    float ms = 0.f;
    HIPC(hipEventElapsedTime(&ms, t.ev[k], t.ev[k + 1]));
    t.ms[t.slot[k]] += ms;
  }
  t.timed = true;
  return DPE_OK;
}

// the prologue of every call: the context quiet, no timings yet, the timer started; a call that restages pts[]
// ends what was resident there
int cloud_begin(DpeContext* c, bool keeps_resident) {
  CloudScratch& v = c->cloud;
  HIPC(host_wait(c));
  if (!keeps_resident) v.resident = CloudResident::None;
  v.timer.timed = false;
  v.timer.on = c->pass.timing;
  v.timer.slot.clear();
  return v.timer.on ? timer_record(c, 0) : DPE_OK;
}

// stages cloud `which` (n points) and enqueues the reduction of its bounds into slot `which`
int cloud_stage(DpeContext* c, int which, const float* pts, size_t n) {
  CloudScratch& v = c->cloud;
  HIPC(v.bounds.ensure(16));
  HIPC(hipMemsetAsync(v.bounds.p + 8 * which, 0, 8 * sizeof(uint32_t), c->stream));
  if (n == 0) return DPE_OK;
  HIPC(v.pts[which].ensure(3 * n));
  HIPC(hipMemcpyAsync(v.pts[which].p, pts, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  LAUNCH(k_cloud_bounds, cloud_blocks(n) < 2048u ? cloud_blocks(n) : 2048u, c, v.pts[which].p, (int)n, v.bounds.p + 8 * which);
  return DPE_OK;
}

// the bounds of the two staged clouds, on the host when it returns
int cloud_bounds_fetch(DpeContext* c, CloudBounds bd[2]) {
  uint32_t raw[16];
  HIPC(hipMemcpyAsync(raw, c->cloud.bounds.p, sizeof raw, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  for (int w = 0; w < 2; ++w) {
    bd[w].finite = raw[8 * w + 6];
    for (int k = 0; k < 3; ++k) { bd[w].lo[k] = cloud_unkey(~raw[8 * w + k]); bd[w].hi[k] = cloud_unkey(raw[8 * w + 3 + k]); }
  }
  return DPE_OK;
}

// count, scan and fill of n staged points over grid g into `sorted` (bucket order), `cnt` = the buckets' ends
int cloud_build(DpeContext* c, const float* pts, size_t n, const CloudGrid& g, int keep_nonfinite, DevArr<int>& cnt,
                float4* sorted) {
  const int nb = (int)(g.mask + 1);
  HIPC(cnt.ensure((size_t)nb));
  HIPC(hipMemsetAsync(cnt.p, 0, (size_t)nb * sizeof(int), c->stream));
  LAUNCH(k_cloud_count, cloud_blocks(n), c, pts, (int)n, g, keep_nonfinite, cnt.p);
  LAUNCH(k_cloud_scan, 1, c, nb, cnt.p);
  LAUNCH(k_cloud_fill, cloud_blocks(n), c, pts, (int)n, g, keep_nonfinite, cnt.p, sorted);
  return DPE_OK;
}

// the levels of the tree over the cnt partials of K doubles in part[0], until one block's result is left: in part[*at]
template <int K>
int tree_reduce(DpeContext* c, DevArr<double> part[2], size_t cnt, int* at) {
  *at = 0;   // part[*at] holds the cnt partials of the level
  while (cnt > 1) {
    const unsigned blocks = cloud_blocks(cnt);
    LAUNCH(k_tree_reduce<K>, blocks, c, part[*at].p, cnt, part[*at ^ 1].p);
    cnt = blocks;
    *at ^= 1;
  }
  return DPE_OK;
}

// out[0..n) = the distances of staged cloud `qi` to staged cloud `ti` (bounds tb), on the host when it returns.
// idx (or null): the matches' indices as well (k_cloud_match instead of k_cloud_query).  Marks build, query, download.
int cloud_direction(DpeContext* c, int qi, size_t n, int ti, size_t m, const CloudBounds& tb, float radius, float* out,
                    int32_t* idx, const char* who) {
  if (n == 0) return DPE_OK;
  CloudScratch& v = c->cloud;
  if (tb.finite == 0) {   // nothing to find: no launch
    const float r2 = radius * radius;
    for (size_t i = 0; i < n; ++i) out[i] = r2;
    if (idx) for (size_t i = 0; i < n; ++i) idx[i] = -1;
    for (int k = 1; k <= 3; ++k) TRY(timer_mark(c, k));
    return DPE_OK;
  }
  CloudGrid g;
  if (!cloud_grid_make(tb.lo, tb.hi, tb.finite, radius, &g)) {
    g_err = std::string(who) + ": radius too small for the cloud's extent";
    return DPE_ERR_ARG;
  }
  HIPC(v.st.ensure(tb.finite));
  HIPC(v.sq.ensure(n));
  HIPC(v.out.ensure(n));
  if (idx) HIPC(v.idx.ensure(n));
  TRY(cloud_build(c, v.pts[ti].p, m, g, 0, v.tcnt, v.st.p));
  TRY(cloud_build(c, v.pts[qi].p, n, g, 1, v.qcnt, v.sq.p));
  TRY(timer_mark(c, 1));
  if (idx) LAUNCH(k_cloud_match, cloud_blocks(n), c, v.sq.p, (int)n, v.st.p, v.tcnt.p, g, v.out.p, v.idx.p);
  else LAUNCH(k_cloud_query, cloud_blocks(n), c, v.sq.p, (int)n, v.st.p, v.tcnt.p, g, v.out.p);
  TRY(timer_mark(c, 2));
  HIPC(hipMemcpyAsync(out, v.out.p, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (idx) HIPC(hipMemcpyAsync(idx, v.idx.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  TRY(timer_mark(c, 3));
  HIPC(hipStreamSynchronize(c->stream));
  return DPE_OK;
}

// two clouds the device can take and a radius; a_out (and b_out when it is needed) where a cloud has points
bool cloud_args_ok(const float* a, size_t n, const float* b, size_t m, float radius, const float* a_out, const float* b_out,
                   bool need_b_out) {
  return n <= (size_t)INT_MAX && m <= (size_t)INT_MAX && (a || n == 0) && (b || m == 0) && (a_out || n == 0) &&
         (!need_b_out || b_out || m == 0) && std::isfinite(radius) && radius > 0.0f;
}

// the two clouds staged once; a_to_b always (with the indices when a_idx is not null), b_to_a when it is not null.
// Timings: [0] stage, then [1] build, [2] query, [3] download summed over the directions
int cloud_run(DpeContext* c, const float* a, size_t n, const float* b, size_t m, float radius, float* a_to_b, int32_t* a_idx,
              float* b_to_a, const char* who) {
  TRY(cloud_begin(c, false));
  TRY(cloud_stage(c, 0, a, n));
  TRY(cloud_stage(c, 1, b, m));
  TRY(timer_mark(c, 0));
  CloudBounds bd[2];
  TRY(cloud_bounds_fetch(c, bd));
  TRY(cloud_direction(c, 0, n, 1, m, bd[1], radius, a_to_b, a_idx, who));
  if (b_to_a) TRY(cloud_direction(c, 1, m, 0, n, bd[0], radius, b_to_a, nullptr, who));
  return timer_finish(c);
}

// dpe_cloud_voxel.  Timings: [0] stage, [1] cells + insert, [2] emit (it holds the host's look at the number of
// voxels), [3] download
int voxel_run(DpeContext* c, const float* xyz, size_t n, const uint8_t* rgb, float voxel, float* out_xyz, uint8_t* out_rgb,
              int32_t* out_first, int32_t* out_count, size_t cap, size_t* k) {
  CloudScratch& s = c->cloud;
  VoxelScratch& v = s.voxel;
  *k = 0;
  TRY(cloud_begin(c, false));
  TRY(cloud_stage(c, 0, xyz, n));
  if (n == 0) { HIPC(hipStreamSynchronize(c->stream)); return DPE_OK; }
  if (rgb) {
    HIPC(v.rgb.ensure(3 * n));
    HIPC(hipMemcpyAsync(v.rgb.p, rgb, 3 * n, hipMemcpyHostToDevice, c->stream));
  }
  TRY(timer_mark(c, 0));
  CloudBounds bd[2];
  TRY(cloud_bounds_fetch(c, bd));
  const size_t finite = bd[0].finite;
  if (finite == 0) return DPE_OK;
  VoxelGrid g;
  if (!voxel_grid_make(bd[0].lo, bd[0].hi, voxel, &g)) {
    g_err = "dpe_cloud_voxel: voxel too small for the cloud's extent";
    return DPE_ERR_ARG;
  }
  // step 1: cells and fractions; step 2: the table
  const size_t slots = (size_t)voxel_slot_count(finite);
  HIPC(v.cell.ensure(n));
  HIPC(v.frac.ensure(3 * n));
  HIPC(v.owner.ensure(slots));
  HIPC(v.first.ensure(slots));
  HIPC(v.count.ensure(slots));
  HIPC(v.sum.ensure(3 * slots));
  if (rgb) HIPC(v.csum.ensure(3 * slots));
  HIPC(v.err.ensure(1));
  HIPC(v.slot_at.ensure(n));
  const size_t nblk = cloud_blocks(n);
  HIPC(v.bcnt.ensure(nblk + 1));
  HIPC(hipMemsetAsync(v.owner.p, 0xFF, slots * sizeof(int), c->stream));
  HIPC(hipMemsetAsync(v.first.p, 0xFF, slots * sizeof(uint32_t), c->stream));
  HIPC(hipMemsetAsync(v.count.p, 0, slots * sizeof(int), c->stream));
  HIPC(hipMemsetAsync(v.sum.p, 0, 3 * slots * sizeof(unsigned long long), c->stream));
  if (rgb) HIPC(hipMemsetAsync(v.csum.p, 0, 3 * slots * sizeof(unsigned long long), c->stream));
  HIPC(hipMemsetAsync(v.err.p, 0, sizeof(uint32_t), c->stream));
  HIPC(hipMemsetAsync(v.slot_at.p, 0xFF, n * sizeof(int), c->stream));
  HIPC(hipMemsetAsync(v.bcnt.p, 0, (nblk + 1) * sizeof(int), c->stream));
  const VoxelTable t = {v.owner.p, v.first.p, v.count.p, v.sum.p, rgb ? v.csum.p : nullptr, (uint32_t)(slots - 1)};
  LAUNCH(k_voxel_cells, nblk, c, s.pts[0].p, (int)n, g, v.cell.p, v.frac.p);
  LAUNCH(k_voxel_insert, nblk, c, v.cell.p, v.frac.p, rgb ? v.rgb.p : nullptr, (int)n, t, v.err.p);
  TRY(timer_mark(c, 1));
  // step 3: the voxels' first points marked, counted per block and scanned; the host looks at their number
  LAUNCH(k_voxel_mark, cloud_blocks(slots), c, t, v.slot_at.p);
  LAUNCH(k_voxel_count, nblk, c, v.slot_at.p, (int)n, v.bcnt.p);
  LAUNCH(k_cloud_scan, 1, c, (int)(nblk + 1), v.bcnt.p);
  uint32_t err = 0;
  int total = 0;
  HIPC(hipMemcpyAsync(&err, v.err.p, sizeof err, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipMemcpyAsync(&total, v.bcnt.p + nblk, sizeof total, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  if (err != 0 || total <= 0) {
    g_err = "dpe_cloud_voxel: the voxel table overflowed";
    return DPE_ERR_STATE;
  }
  *k = (size_t)total;
  if ((size_t)total > cap) {
    g_err = "dpe_cloud_voxel: output buffers too small for the voxels";
    return DPE_ERR_ARG;
  }
  const size_t nv = (size_t)total;
  HIPC(v.out_xyz.ensure(3 * nv));
  if (rgb) HIPC(v.out_rgb.ensure(3 * nv));
  HIPC(v.out_first.ensure(nv));
  HIPC(v.out_count.ensure(nv));
  LAUNCH(k_voxel_fill, nblk, c, v.slot_at.p, (int)n, v.bcnt.p, v.cell.p, g, t, v.out_xyz.p, rgb ? v.out_rgb.p : nullptr,
         v.out_first.p, v.out_count.p);
  TRY(timer_mark(c, 2));
  HIPC(hipMemcpyAsync(out_xyz, v.out_xyz.p, 3 * nv * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (rgb) HIPC(hipMemcpyAsync(out_rgb, v.out_rgb.p, 3 * nv, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipMemcpyAsync(out_first, v.out_first.p, nv * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPC(hipMemcpyAsync(out_count, v.out_count.p, nv * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  TRY(timer_mark(c, 3));
  HIPC(hipStreamSynchronize(c->stream));
  return timer_finish(c);
}

// dpe_cloud_icp_stage: both clouds and the target's grid for `radius` resident.  No timings
int icp_stage(DpeContext* c, const float* src, size_t n, const float* tgt, size_t m, float radius) {
  CloudScratch& v = c->cloud;
  IcpStage& s = v.icp;
  TRY(cloud_begin(c, false));
  TRY(cloud_stage(c, 0, src, n));
  TRY(cloud_stage(c, 1, tgt, m));
  CloudBounds bd[2];
  TRY(cloud_bounds_fetch(c, bd));
  s.n = n;
  s.m = m;
  s.tfinite = bd[1].finite;
  for (int a = 0; a < 3; ++a) {
    s.os[a] = bd[0].finite ? (double)bd[0].lo[a] : 0.0;
    s.ot[a] = bd[1].finite ? (double)bd[1].lo[a] : 0.0;
  }
  if (n > 0 && bd[1].finite > 0) {
    if (!cloud_grid_make(bd[1].lo, bd[1].hi, bd[1].finite, radius, &s.grid)) {
      g_err = "dpe_cloud_icp_stage: radius too small for the cloud's extent";
      return DPE_ERR_ARG;
    }
    HIPC(v.st.ensure(bd[1].finite));
    TRY(cloud_build(c, v.pts[1].p, m, s.grid, 0, v.tcnt, v.st.p));
    // what a step writes
    const size_t blocks = cloud_blocks(n);
    HIPC(s.moved.ensure(3 * n));
    HIPC(v.sq.ensure(n));
    HIPC(v.out.ensure(n));
    HIPC(v.idx.ensure(n));
    HIPC(s.part[0].ensure(blocks * kIcpTerms));
    HIPC(s.part[1].ensure((size_t)cloud_blocks(blocks) * kIcpTerms));
    HIPC(s.matched.ensure(1));
    HIPC(hipStreamSynchronize(c->stream));
  }
  v.resident = CloudResident::IcpPair;
  return DPE_OK;
}

// dpe_cloud_icp_step over the staged pair.  Timings: [0] apply + build, [1] match, [2] sums, [3] download
int icp_step(DpeContext* c, const double* T, DpeIcpSums* out) {
  CloudScratch& v = c->cloud;
  IcpStage& st = v.icp;
  TRY(cloud_begin(c, true));
  DpeIcpSums s;
  memset(&s, 0, sizeof s);
  const size_t n = st.n;
  if (n == 0 || st.tfinite == 0) { *out = s; return DPE_OK; }   // nothing to match: no launch
  IcpXf xf;
  memcpy(xf.m, T, sizeof xf.m);
  IcpOrigins org;
  memcpy(org.s, st.os, sizeof org.s);
  memcpy(org.t, st.ot, sizeof org.t);
  const CloudGrid& g = st.grid;
  HIPC(hipMemsetAsync(st.matched.p, 0, sizeof(unsigned long long), c->stream));
  LAUNCH(k_icp_apply, cloud_blocks(n), c, v.pts[0].p, (int)n, xf, st.moved.p);
  TRY(cloud_build(c, st.moved.p, n, g, 1, v.qcnt, v.sq.p));
  TRY(timer_mark(c, 0));
  LAUNCH(k_cloud_match, cloud_blocks(n), c, v.sq.p, (int)n, v.st.p, v.tcnt.p, g, v.out.p, v.idx.p);
  TRY(timer_mark(c, 1));
  LAUNCH(k_icp_terms, cloud_blocks(n), c, v.pts[0].p, (int)n, v.pts[1].p, v.idx.p, v.out.p, org, st.part[0].p, st.matched.p);
  int at;
  TRY(tree_reduce<kIcpTerms>(c, st.part, cloud_blocks(n), &at));
  TRY(timer_mark(c, 2));
  double sums[kIcpTerms];
  unsigned long long matched = 0;
  HIPC(hipMemcpyAsync(sums, st.part[at].p, sizeof sums, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipMemcpyAsync(&matched, st.matched.p, sizeof matched, hipMemcpyDeviceToHost, c->stream));
  TRY(timer_mark(c, 3));
  HIPC(hipStreamSynchronize(c->stream));
  s.matched = (long long)matched;
  s.d2 = sums[0];
  for (int k = 0; k < 3; ++k) { s.a[k] = sums[1 + k]; s.b[k] = sums[4 + k]; }
  for (int k = 0; k < 9; ++k) s.ab[k] = sums[7 + k];
  *out = s;
  return timer_finish(c);
}

// dpe_cloud_render_stage: the scan resident in pts[0], with its normals when they are given.  Timings: [0] stage
int render_stage(DpeContext* c, const float* xyz, const float* normals, size_t n) {
  CloudScratch& v = c->cloud;
  TRY(cloud_begin(c, false));
  if (n > 0) {
    HIPC(v.pts[0].ensure(3 * n));
    HIPC(hipMemcpyAsync(v.pts[0].p, xyz, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (normals) {
      HIPC(v.normals.staged.ensure(3 * n));
      HIPC(hipMemcpyAsync(v.normals.staged.p, normals, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    }
  }
  TRY(timer_mark(c, 0));
  HIPC(hipStreamSynchronize(c->stream));
  v.render.n = n;
  v.normals.has_staged = normals != nullptr;
  v.resident = CloudResident::RenderScan;
  return timer_finish(c);
}

// dpe_cloud_render_view and dpe_cloud_render_view_normals of the staged scan.  A plain view invalidates the resident
// normal map, which would belong to another depth map; a view with normals leaves both.  Timings: [1] render,
// [3] download
int render_view(DpeContext* c, const DpeCamera& cam, int splat, bool with_normals, float* depth_out, float* normal_out) {
  RenderStage& r = c->cloud.render;
  NormalScratch& s = c->cloud.normals;
  TRY(cloud_begin(c, true));
  const size_t npx = (size_t)cam.width * (size_t)cam.height, n = r.n;
  const float* pts = c->cloud.pts[0].p;
  r.map_w = r.map_h = 0;   // the old maps go with the first launch
  s.map_w = s.map_h = 0;
  HIPC(r.map.ensure(npx));
  if (with_normals) {
    HIPC(s.zb.ensure(npx));
    HIPC(s.winner.ensure(npx));
    HIPC(s.map.ensure(3 * npx));
    LAUNCH(k_render_clear<unsigned long long>, cloud_blocks(npx), c, s.zb.p, npx);
    if (n > 0) LAUNCH(k_render_splat<unsigned long long>, cloud_blocks(n), c, pts, (int)n, cam, splat, s.zb.p);
    LAUNCH(k_render_finish_idx, cloud_blocks(npx), c, s.zb.p, npx, r.map.p, s.winner.p);
    LAUNCH(k_render_normals, cloud_blocks(npx), c, pts, s.staged.p, s.winner.p, npx, cam, s.map.p);
  } else {
    LAUNCH(k_render_clear<uint32_t>, cloud_blocks(npx), c, r.map.p, npx);
    if (n > 0) LAUNCH(k_render_splat<uint32_t>, cloud_blocks(n), c, pts, (int)n, cam, splat, r.map.p);
    LAUNCH(k_render_finish, cloud_blocks(npx), c, r.map.p, npx);
  }
  TRY(timer_mark(c, 1));
  if (depth_out) HIPC(hipMemcpyAsync(depth_out, r.map.p, npx * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (normal_out) HIPC(hipMemcpyAsync(normal_out, s.map.p, 3 * npx * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  TRY(timer_mark(c, 3));
  HIPC(hipStreamSynchronize(c->stream));
  r.map_w = cam.width;
  r.map_h = cam.height;
  if (with_normals) { s.map_w = cam.width; s.map_h = cam.height; }
  return timer_finish(c);
}

// dpe_depth_score and dpe_normal_score; gt == nullptr: against the resident map `resident`.  Timings: [0] upload,
// [2] score, [3] download
template <typename M>
int score_run(DpeContext* c, const float* est, const float* gt, const float* resident, int w, int h, const typename M::Taus& T,
              typename M::Score* out, float* err) {
  ScoreScratch& v = c->cloud.score;
  TRY(cloud_begin(c, true));
  const size_t npx = (size_t)w * (size_t)h, blocks = cloud_blocks(npx), nval = M::kChannels * npx;
  HIPC(v.est.ensure(nval));
  if (gt) HIPC(v.gt.ensure(nval));
  if (err) HIPC(v.err.ensure(npx));
  HIPC(v.part[0].ensure(blocks * M::kTerms));
  HIPC(v.part[1].ensure((size_t)cloud_blocks(blocks) * M::kTerms));
  HIPC(v.cnt.ensure(M::kCounters));
  const float* edges = nullptr;
  if constexpr (M::kBins > 0) {
    DevArr<float>& e = c->cloud.normals.edges;
    if (e.n == 0) {   // the table of the one host function, uploaded once per context
      float E[M::kBins];
      M::edges(E);
      HIPC(e.ensure(M::kBins));
      HIPC(hipMemcpyAsync(e.p, E, sizeof E, hipMemcpyHostToDevice, c->stream));
      HIPC(hipStreamSynchronize(c->stream));   // E leaves the stack
    }
    edges = e.p;
  }
  HIPC(hipMemcpyAsync(v.est.p, est, nval * sizeof(float), hipMemcpyHostToDevice, c->stream));
  if (gt) HIPC(hipMemcpyAsync(v.gt.p, gt, nval * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPC(hipMemsetAsync(v.cnt.p, 0, M::kCounters * sizeof(unsigned long long), c->stream));
  TRY(timer_mark(c, 0));
  LAUNCH(k_map_score<M>, blocks, c, v.est.p, gt ? v.gt.p : resident, npx, T, v.part[0].p, v.cnt.p,
         err ? v.err.p : nullptr, edges);
  int at;
  TRY(tree_reduce<M::kTerms>(c, v.part, blocks, &at));
  TRY(timer_mark(c, 2));
  double sums[M::kTerms];
  unsigned long long counts[M::kCounters];
  HIPC(hipMemcpyAsync(sums, v.part[at].p, sizeof sums, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipMemcpyAsync(counts, v.cnt.p, sizeof counts, hipMemcpyDeviceToHost, c->stream));
  if (err) HIPC(hipMemcpyAsync(err, v.err.p, npx * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  TRY(timer_mark(c, 3));
  HIPC(hipStreamSynchronize(c->stream));
  *out = score_of<M>(npx, T.n, counts, sums);
  return timer_finish(c);
}

// the camera and the splat of a render, and the scan staged before it (`stage`: the call that stages)
int render_enter(DpeContext* c, const DpeCamera* cam, int splat, const char* who, const char* stage) {
  const bool ok = cam && cam->width >= 1 && cam->height >= 1 && splat >= 0 && splat <= DPE_DEPTH_MAX_SPLAT;
  TRY(enter(c, ok, (std::string(who) + ": bad argument").c_str()));
  if (c->cloud.resident != CloudResident::RenderScan) {
    g_err = std::string(who) + ": no staged cloud (" + stage + " comes first)";
    return DPE_ERR_STATE;
  }
  return DPE_OK;
}

// a score without gt: the resident map (map_w x map_h, 0: none, rendered by `view`) must be there and of the size
int score_resident_ok(const float* gt, int map_w, int map_h, int w, int h, const char* who, const char* view) {
  if (gt) return DPE_OK;
  if (map_w == 0) {
    g_err = std::string(who) + ": no rendered map (" + view + " comes first, or pass gt)";
    return DPE_ERR_STATE;
  }
  if (map_w != w || map_h != h) {
    g_err = std::string(who) + ": the size differs from the rendered map's";
    return DPE_ERR_ARG;
  }
  return DPE_OK;
}

// dpe_cloud_normals.  Timings: [0] stage, [1] build, [2] normals, [3] download
int normals_run(DpeContext* c, const float* xyz, size_t n, float radius, int min_nb, float* normal_out, int32_t* count_out,
                long long* sums_out) {
  CloudScratch& v = c->cloud;
  NormalScratch& s = v.normals;
  TRY(cloud_begin(c, false));
  TRY(cloud_stage(c, 0, xyz, n));
  if (n == 0) { HIPC(hipStreamSynchronize(c->stream)); return DPE_OK; }
  TRY(timer_mark(c, 0));
  CloudBounds bd[2];
  TRY(cloud_bounds_fetch(c, bd));
  const size_t finite = bd[0].finite;
  if (finite == 0) {   // no neighbour anywhere: no launch
    memset(normal_out, 0, 3 * n * sizeof(float));
    memset(count_out, 0, n * sizeof(int32_t));
    if (sums_out) memset(sums_out, 0, (size_t)kNormalSums * n * sizeof(long long));
    return DPE_OK;
  }
  CloudGrid g;
  if (!cloud_grid_make(bd[0].lo, bd[0].hi, finite, radius, &g)) {
    g_err = "dpe_cloud_normals: radius too small for the cloud's extent";
    return DPE_ERR_ARG;
  }
  HIPC(v.st.ensure(finite));
  HIPC(s.normal.ensure(3 * n));
  HIPC(s.count.ensure(n));
  if (sums_out) HIPC(s.sums.ensure((size_t)kNormalSums * n));
  // a non-finite point has no thread: its outputs are the zeros written here
  HIPC(hipMemsetAsync(s.normal.p, 0, 3 * n * sizeof(float), c->stream));
  HIPC(hipMemsetAsync(s.count.p, 0, n * sizeof(int), c->stream));
  if (sums_out) HIPC(hipMemsetAsync(s.sums.p, 0, (size_t)kNormalSums * n * sizeof(long long), c->stream));
  TRY(cloud_build(c, v.pts[0].p, n, g, 0, v.tcnt, v.st.p));
  TRY(timer_mark(c, 1));
  LAUNCH(k_cloud_normal, cloud_blocks(finite), c, v.st.p, (int)finite, v.tcnt.p, g, normal_scale(radius), min_nb, s.normal.p,
         s.count.p, sums_out ? s.sums.p : nullptr);
  TRY(timer_mark(c, 2));
  HIPC(hipMemcpyAsync(normal_out, s.normal.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPC(hipMemcpyAsync(count_out, s.count.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (sums_out)
    HIPC(hipMemcpyAsync(sums_out, s.sums.p, (size_t)kNormalSums * n * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  TRY(timer_mark(c, 3));
  HIPC(hipStreamSynchronize(c->stream));
  return timer_finish(c);
}

}  // namespace

extern "C" int dpe_cloud_normals(DpeContext* c, const float* xyz, size_t n, float radius, int min_nb, float* normal_out,
                                 int32_t* count_out, long long* sums_out) {
  const bool ok = cloud_args_ok(xyz, n, nullptr, 0, radius, normal_out, nullptr, false) && (count_out || n == 0) &&
                  min_nb >= kNormalMinNb;
  TRY(enter(c, ok, "dpe_cloud_normals: bad argument"));
  return normals_run(c, xyz, n, radius, min_nb, normal_out, count_out, sums_out);
}

extern "C" int dpe_cloud_render_stage_normals(DpeContext* c, const float* xyz, const float* normals, size_t n) {
  float none = 0.f;   // n == 0: no entry, and the staging still counts as one with normals
  TRY(enter(c, n <= (size_t)INT_MAX && ((xyz && normals) || n == 0), "dpe_cloud_render_stage_normals: bad argument"));
  return render_stage(c, xyz, normals ? normals : &none, n);
}

extern "C" int dpe_cloud_render_view_normals(DpeContext* c, const DpeCamera* cam, int splat, float* depth_out,
                                             float* normal_out) {
  TRY(render_enter(c, cam, splat, "dpe_cloud_render_view_normals", "dpe_cloud_render_stage_normals"));
  if (!c->cloud.normals.has_staged) {
    g_err = "dpe_cloud_render_view_normals: no staged normals (dpe_cloud_render_stage_normals comes first)";
    return DPE_ERR_STATE;
  }
  return render_view(c, *cam, splat, true, depth_out, normal_out);
}

extern "C" int dpe_normal_score(DpeContext* c, const float* est, const float* gt, int w, int h, const float* cos_tau, int n_tau,
                                DpeNormalScore* out, float* err) {
  bool ok = est && w >= 1 && h >= 1 && cos_tau && n_tau >= 1 && n_tau <= DPE_NORMAL_MAX_TAU && out;
  NormalTaus T;
  memset(&T, 0, sizeof T);
  for (int k = 0; ok && k < n_tau; ++k) {
    ok = std::isfinite(cos_tau[k]) && cos_tau[k] >= -1.0f && cos_tau[k] <= 1.0f;
    T.c[k] = cos_tau[k];
  }
  T.n = n_tau;
  TRY(enter(c, ok, "dpe_normal_score: bad argument"));
  const NormalScratch& s = c->cloud.normals;
  TRY(score_resident_ok(gt, s.map_w, s.map_h, w, h, "dpe_normal_score", "dpe_cloud_render_view_normals"));
  return score_run<NormalMetric>(c, est, gt, s.map.p, w, h, T, out, err);
}

extern "C" int dpe_cloud_render_stage(DpeContext* c, const float* xyz, size_t n) {
  TRY(enter(c, n <= (size_t)INT_MAX && (xyz || n == 0), "dpe_cloud_render_stage: bad argument"));
  return render_stage(c, xyz, nullptr, n);
}

extern "C" int dpe_cloud_render_view(DpeContext* c, const DpeCamera* cam, int splat, float* depth_out) {
  TRY(render_enter(c, cam, splat, "dpe_cloud_render_view", "dpe_cloud_render_stage"));
  return render_view(c, *cam, splat, false, depth_out, nullptr);
}

extern "C" int dpe_depth_score(DpeContext* c, const float* est, const float* gt, int w, int h, const float* tau, int n_tau,
                               int mode, DpeDepthScore* out, float* err) {
  bool ok = est && w >= 1 && h >= 1 && tau && n_tau >= 1 && n_tau <= DPE_DEPTH_MAX_TAU && out &&
            (mode == DPE_DEPTH_TAU_ABS || mode == DPE_DEPTH_TAU_REL);
  DepthTaus T;
  memset(&T, 0, sizeof T);
  for (int k = 0; ok && k < n_tau; ++k) {
    ok = std::isfinite(tau[k]) && tau[k] >= 0.0f;
    T.tau[k] = tau[k];
  }
  T.n = n_tau;
  T.mode = mode;
  TRY(enter(c, ok, "dpe_depth_score: bad argument"));
  const RenderStage& r = c->cloud.render;
  TRY(score_resident_ok(gt, r.map_w, r.map_h, w, h, "dpe_depth_score", "dpe_cloud_render_view"));
  return score_run<DepthMetric>(c, est, gt, reinterpret_cast<const float*>(r.map.p), w, h, T, out, err);
}

extern "C" int dpe_cloud_nn_index(DpeContext* c, const float* query, size_t n, const float* target, size_t m, float radius,
                                  float* d2_out, int32_t* idx_out) {
  const bool ok = cloud_args_ok(query, n, target, m, radius, d2_out, nullptr, false) && (idx_out || n == 0);
  TRY(enter(c, ok, "dpe_cloud_nn_index: bad argument"));
  int32_t none = -1;   // n == 0: no entry, and the call still stages as one with indices
  return cloud_run(c, query, n, target, m, radius, d2_out, idx_out ? idx_out : &none, nullptr, "dpe_cloud_nn_index");
}

extern "C" int dpe_cloud_icp_stage(DpeContext* c, const float* src, size_t n, const float* tgt, size_t m, float radius) {
  // the stage writes nothing for the caller: the source stands in for the output cloud_args_ok asks for
  TRY(enter(c, cloud_args_ok(src, n, tgt, m, radius, src, nullptr, false), "dpe_cloud_icp_stage: bad argument"));
  return icp_stage(c, src, n, tgt, m, radius);
}

extern "C" int dpe_cloud_icp_step(DpeContext* c, const double* T, DpeIcpSums* out) {
  TRY(enter(c, T && out, "dpe_cloud_icp_step: bad argument"));
  if (c->cloud.resident != CloudResident::IcpPair) {
    g_err = "dpe_cloud_icp_step: no staged pair (dpe_cloud_icp_stage comes first)";
    return DPE_ERR_STATE;
  }
  return icp_step(c, T, out);
}

extern "C" int dpe_cloud_voxel(DpeContext* c, const float* xyz, size_t n, const uint8_t* rgb, float voxel, float* out_xyz,
                               uint8_t* out_rgb, int32_t* out_first, int32_t* out_count, size_t cap, size_t* k) {
  const bool ok = n <= (size_t)INT_MAX && (xyz || n == 0) && k && std::isfinite(voxel) && voxel > 0.0f &&
                  (cap == 0 || (out_xyz && out_first && out_count && (!rgb || out_rgb)));
  TRY(enter(c, ok, "dpe_cloud_voxel: bad argument"));
  return voxel_run(c, xyz, n, rgb, voxel, out_xyz, out_rgb, out_first, out_count, cap, k);
}

extern "C" int dpe_cloud_nn(DpeContext* c, const float* query, size_t n, const float* target, size_t m, float radius,
                            float* d2_out) {
  TRY(enter(c, cloud_args_ok(query, n, target, m, radius, d2_out, nullptr, false), "dpe_cloud_nn: bad argument"));
  return cloud_run(c, query, n, target, m, radius, d2_out, nullptr, nullptr, "dpe_cloud_nn");
}

extern "C" int dpe_cloud_nn_pair(DpeContext* c, const float* a, size_t n, const float* b, size_t m, float radius,
                                 float* a_to_b, float* b_to_a) {
  TRY(enter(c, cloud_args_ok(a, n, b, m, radius, a_to_b, b_to_a, true), "dpe_cloud_nn_pair: bad argument"));
  float none = 0.f;   // m == 0: b_to_a has no entry, and the second direction still runs as one
  return cloud_run(c, a, n, b, m, radius, a_to_b, nullptr, b_to_a ? b_to_a : &none, "dpe_cloud_nn_pair");
}

extern "C" int dpe_cloud_last_timings(DpeContext* c, float* ms, int n) {
  if (!c || !ms || !c->cloud.timer.timed) return 0;
  int k = 0;
  for (; k < n && k < 4; ++k) ms[k] = c->cloud.timer.ms[k];
  return k;
}
