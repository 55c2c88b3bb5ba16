// dpe_cloud.hip -- the cloud evaluation's distances (dpe_cloud_nn, dpe_cloud_nn_pair), the voxel
// down-sampling (dpe_cloud_voxel) and the registration's device half (dpe_cloud_nn_index, dpe_cloud_icp_stage,
// dpe_cloud_icp_step) and the depth-map evaluation (dpe_cloud_render_stage, dpe_cloud_render_view, dpe_depth_score)
// of include/dpe_mvs.h: the kernels of pass_cloud.h, pass_voxel.h, pass_register.h and pass_render.h over
// the context's cloud scratch.  A unit of libdpe_mvs.so; the concurrency
// contract is dpe_mvs.hip's (dpe_entry.h): these calls wait until the context is quiet, use its stream and
// return with it synchronised.
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
#include "dpe_entry.h"
#include "dpe_context.h"

using namespace dpe;

static std::atomic<long long> g_cloud_launches{0};

extern "C" long long dpe_cloud_launches(void) { return g_cloud_launches.load(); }

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

// the timing events of this section, made at the first timed call
int cloud_events(DpeContext* c) {
  CloudScratch& v = c->cloud;
  while (v.ev.size() < 8) {
    Event e;
    HIPC(e.create(hipEventDefault));
    v.ev.push_back(std::move(e));
  }
  return DPE_OK;
}

unsigned cloud_blocks(size_t n) { return (unsigned)((n + kCloudBlock - 1) / kCloudBlock); }

// stages cloud `which` (n points) and enqueues the reduction of its bounds into slot `which`
int cloud_stage(DpeContext* c, int which, const float* pts, size_t n) {
  CloudScratch& v = c->cloud;
  HIPC(v.bounds.ensure(16));
  HIPC(hipMemsetAsync(v.bounds.p + 8 * which, 0, 8 * sizeof(uint32_t), c->stream));
  if (n == 0) return DPE_OK;
  HIPC(v.pts[which].ensure(3 * n));
  HIPC(hipMemcpyAsync(v.pts[which].p, pts, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  const unsigned grid = cloud_blocks(n) < 2048u ? cloud_blocks(n) : 2048u;
  k_cloud_bounds<<<grid, kCloudBlock, 0, c->stream>>>(v.pts[which].p, (int)n, v.bounds.p + 8 * which);
  HIPC(hipGetLastError());
  g_cloud_launches += 1;
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
  k_cloud_count<<<cloud_blocks(n), kCloudBlock, 0, c->stream>>>(pts, (int)n, g, keep_nonfinite, cnt.p);
  HIPC(hipGetLastError());
  k_cloud_scan<<<1, kCloudBlock, 0, c->stream>>>(nb, cnt.p);
  HIPC(hipGetLastError());
  k_cloud_fill<<<cloud_blocks(n), kCloudBlock, 0, c->stream>>>(pts, (int)n, g, keep_nonfinite, cnt.p, sorted);
  HIPC(hipGetLastError());
  g_cloud_launches += 3;
  return DPE_OK;
}

// out[0..n) = the distances of staged cloud `qi` to staged cloud `ti` (bounds tb), on the host when it returns.
// idx (or null): the matches' indices as well (k_cloud_match instead of k_cloud_query).
// ev: the three timing events of this direction (end of build, query, download), or null.
int cloud_direction(DpeContext* c, int qi, size_t n, int ti, size_t m, const CloudBounds& tb, float radius, float* out,
                    int32_t* idx, Event* ev, const char* who) {
  if (n == 0) return DPE_OK;
  CloudScratch& v = c->cloud;
  if (tb.finite == 0) {   // nothing to find: no launch
    const float r2 = radius * radius;
    for (size_t i = 0; i < n; ++i) out[i] = r2;
    if (idx) for (size_t i = 0; i < n; ++i) idx[i] = -1;
    if (ev) for (int k = 0; k < 3; ++k) HIPC(hipEventRecord(ev[k], c->stream));
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
  if (ev) HIPC(hipEventRecord(ev[0], c->stream));
  if (idx) k_cloud_match<<<cloud_blocks(n), kCloudBlock, 0, c->stream>>>(v.sq.p, (int)n, v.st.p, v.tcnt.p, g, v.out.p, v.idx.p);
  else k_cloud_query<<<cloud_blocks(n), kCloudBlock, 0, c->stream>>>(v.sq.p, (int)n, v.st.p, v.tcnt.p, g, v.out.p);
  HIPC(hipGetLastError());
  g_cloud_launches += 1;
  if (ev) HIPC(hipEventRecord(ev[1], c->stream));
  HIPC(hipMemcpyAsync(out, v.out.p, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (idx) HIPC(hipMemcpyAsync(idx, v.idx.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (ev) HIPC(hipEventRecord(ev[2], c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  return DPE_OK;
}

bool cloud_args_ok(const float* a, size_t n, const float* b, size_t m, float radius, const float* a_out, const float* b_out,
                   bool need_b_out) {
  return n <= (size_t)INT_MAX && m <= (size_t)INT_MAX && (a || n == 0) && (b || m == 0) && (a_out || n == 0) &&
         (!need_b_out || b_out || m == 0) && std::isfinite(radius) && radius > 0.0f;
}

// the two clouds staged once; a_to_b always (with the indices when a_idx is not null), b_to_a when it is not null
int cloud_run(DpeContext* c, const float* a, size_t n, const float* b, size_t m, float radius, float* a_to_b, int32_t* a_idx,
              float* b_to_a, const char* who) {
  CloudScratch& v = c->cloud;
  HIPC(host_wait(c));
  const bool timing = c->pass.timing;
  v.timed = false;
  v.icp_staged = false;
  v.render_staged = false;
  if (timing) TRY(cloud_events(c));
  if (timing) HIPC(hipEventRecord(v.ev[0], c->stream));
  TRY(cloud_stage(c, 0, a, n));
  TRY(cloud_stage(c, 1, b, m));
  if (timing) HIPC(hipEventRecord(v.ev[1], c->stream));
  CloudBounds bd[2];
  TRY(cloud_bounds_fetch(c, bd));
  TRY(cloud_direction(c, 0, n, 1, m, bd[1], radius, a_to_b, a_idx, timing ? &v.ev[2] : nullptr, who));
  if (b_to_a) TRY(cloud_direction(c, 1, m, 0, n, bd[0], radius, b_to_a, nullptr, timing ? &v.ev[5] : nullptr, who));
  if (timing) {
    // [0] stage, [1] build, [2] query, [3] download; an empty direction records nothing
    const bool ran[2] = {n > 0, b_to_a && m > 0};
    float ms = 0.f;
    for (float& t : v.ms) t = 0.f;
    HIPC(hipEventElapsedTime(&ms, v.ev[0], v.ev[1]));
    v.ms[0] = ms;
    int prev = 1;
    for (int d = 0; d < 2; ++d) {
      if (!ran[d]) continue;
      for (int k = 0; k < 3; ++k) {
        HIPC(hipEventSynchronize(v.ev[2 + 3 * d + k]));
        HIPC(hipEventElapsedTime(&ms, v.ev[prev], v.ev[2 + 3 * d + k]));
        v.ms[1 + k] += ms;
        prev = 2 + 3 * d + k;
      }
    }
    v.timed = true;
  }
  return DPE_OK;
}

unsigned voxel_blocks(size_t n) { return (unsigned)((n + kVoxelBlock - 1) / kVoxelBlock); }

// dpe_cloud_voxel after its prologue.  Timing events: [0] start, [1] staged, [2] cells + insert, [3] emit,
// [4] download (the emit part holds the host's look at the number of voxels).
int voxel_run(DpeContext* c, const float* xyz, size_t n, const uint8_t* rgb, float voxel, float* out_xyz, uint8_t* out_rgb,
              int32_t* out_first, int32_t* out_count, size_t cap, size_t* k) {
  CloudScratch& v = c->cloud;
  *k = 0;
  HIPC(host_wait(c));
  const bool timing = c->pass.timing;
  v.timed = false;
  v.icp_staged = false;
  v.render_staged = false;
  if (timing) TRY(cloud_events(c));
  if (timing) HIPC(hipEventRecord(v.ev[0], c->stream));
  TRY(cloud_stage(c, 0, xyz, n));
  if (n == 0) { HIPC(hipStreamSynchronize(c->stream)); return DPE_OK; }
  if (rgb) {
    HIPC(v.vrgb.ensure(3 * n));
    HIPC(hipMemcpyAsync(v.vrgb.p, rgb, 3 * n, hipMemcpyHostToDevice, c->stream));
  }
  if (timing) HIPC(hipEventRecord(v.ev[1], c->stream));
  uint32_t raw[8];
  HIPC(hipMemcpyAsync(raw, v.bounds.p, sizeof raw, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  const size_t finite = raw[6];
  if (finite == 0) return DPE_OK;
  float lo[3], hi[3];
  for (int a = 0; a < 3; ++a) { lo[a] = cloud_unkey(~raw[a]); hi[a] = cloud_unkey(raw[3 + a]); }
  VoxelGrid g;
  if (!voxel_grid_make(lo, hi, voxel, &g)) {
    g_err = "dpe_cloud_voxel: voxel too small for the cloud's extent";
    return DPE_ERR_ARG;
  }
  // step 1: cells and fractions; step 2: the table
  const size_t slots = (size_t)voxel_slot_count(finite);
  HIPC(v.vcell.ensure(n));
  HIPC(v.vfrac.ensure(3 * n));
  HIPC(v.vowner.ensure(slots));
  HIPC(v.vfirst.ensure(slots));
  HIPC(v.vcount.ensure(slots));
  HIPC(v.vsum.ensure(3 * slots));
  if (rgb) HIPC(v.vcsum.ensure(3 * slots));
  HIPC(v.verr.ensure(1));
  HIPC(v.vslot_at.ensure(n));
  const size_t nblk = voxel_blocks(n);
  HIPC(v.vbcnt.ensure(nblk + 1));
  HIPC(hipMemsetAsync(v.vowner.p, 0xFF, slots * sizeof(int), c->stream));
  HIPC(hipMemsetAsync(v.vfirst.p, 0xFF, slots * sizeof(uint32_t), c->stream));
  HIPC(hipMemsetAsync(v.vcount.p, 0, slots * sizeof(int), c->stream));
  HIPC(hipMemsetAsync(v.vsum.p, 0, 3 * slots * sizeof(unsigned long long), c->stream));
  if (rgb) HIPC(hipMemsetAsync(v.vcsum.p, 0, 3 * slots * sizeof(unsigned long long), c->stream));
  HIPC(hipMemsetAsync(v.verr.p, 0, sizeof(uint32_t), c->stream));
  HIPC(hipMemsetAsync(v.vslot_at.p, 0xFF, n * sizeof(int), c->stream));
  HIPC(hipMemsetAsync(v.vbcnt.p, 0, (nblk + 1) * sizeof(int), c->stream));
  const VoxelTable t = {v.vowner.p, v.vfirst.p, v.vcount.p, v.vsum.p, rgb ? v.vcsum.p : nullptr, (uint32_t)(slots - 1)};
  k_voxel_cells<<<voxel_blocks(n), kVoxelBlock, 0, c->stream>>>(v.pts[0].p, (int)n, g, v.vcell.p, v.vfrac.p);
  HIPC(hipGetLastError());
  k_voxel_insert<<<voxel_blocks(n), kVoxelBlock, 0, c->stream>>>(v.vcell.p, v.vfrac.p, rgb ? v.vrgb.p : nullptr, (int)n, t, v.verr.p);
  HIPC(hipGetLastError());
  g_cloud_launches += 2;
  if (timing) HIPC(hipEventRecord(v.ev[2], c->stream));
  // step 3: the voxels' first points marked, counted per block and scanned; the host looks at their number
  k_voxel_mark<<<voxel_blocks(slots), kVoxelBlock, 0, c->stream>>>(t, v.vslot_at.p);
  HIPC(hipGetLastError());
  k_voxel_count<<<voxel_blocks(n), kVoxelBlock, 0, c->stream>>>(v.vslot_at.p, (int)n, v.vbcnt.p);
  HIPC(hipGetLastError());
  k_cloud_scan<<<1, kCloudBlock, 0, c->stream>>>((int)(nblk + 1), v.vbcnt.p);
  HIPC(hipGetLastError());
  g_cloud_launches += 3;
  uint32_t err = 0;
  int total = 0;
  HIPC(hipMemcpyAsync(&err, v.verr.p, sizeof err, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipMemcpyAsync(&total, v.vbcnt.p + nblk, sizeof total, hipMemcpyDeviceToHost, c->stream));
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
  HIPC(v.vout_xyz.ensure(3 * nv));
  if (rgb) HIPC(v.vout_rgb.ensure(3 * nv));
  HIPC(v.vout_first.ensure(nv));
  HIPC(v.vout_count.ensure(nv));
  k_voxel_fill<<<voxel_blocks(n), kVoxelBlock, 0, c->stream>>>(v.vslot_at.p, (int)n, v.vbcnt.p, v.vcell.p, g, t, v.vout_xyz.p,
                                                               rgb ? v.vout_rgb.p : nullptr, v.vout_first.p, v.vout_count.p);
  HIPC(hipGetLastError());
  g_cloud_launches += 1;
  if (timing) HIPC(hipEventRecord(v.ev[3], c->stream));
  HIPC(hipMemcpyAsync(out_xyz, v.vout_xyz.p, 3 * nv * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (rgb) HIPC(hipMemcpyAsync(out_rgb, v.vout_rgb.p, 3 * nv, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipMemcpyAsync(out_first, v.vout_first.p, nv * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPC(hipMemcpyAsync(out_count, v.vout_count.p, nv * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (timing) HIPC(hipEventRecord(v.ev[4], c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  if (timing) {
    for (int e = 0; e < 4; ++e) HIPC(hipEventElapsedTime(&v.ms[e], v.ev[e], v.ev[e + 1]));
    v.timed = true;
  }
  return DPE_OK;
}

// dpe_cloud_icp_stage after its prologue: both clouds and the target's grid for `radius` resident
int icp_stage(DpeContext* c, const float* src, size_t n, const float* tgt, size_t m, float radius) {
  CloudScratch& v = c->cloud;
  HIPC(host_wait(c));
  v.timed = false;
  v.icp_staged = false;
  v.render_staged = false;
  TRY(cloud_stage(c, 0, src, n));
  TRY(cloud_stage(c, 1, tgt, m));
  CloudBounds bd[2];
  TRY(cloud_bounds_fetch(c, bd));
  v.icp_n = n;
  v.icp_m = m;
  v.icp_tfinite = bd[1].finite;
  for (int a = 0; a < 3; ++a) {
    v.icp_os[a] = bd[0].finite ? (double)bd[0].lo[a] : 0.0;
    v.icp_ot[a] = bd[1].finite ? (double)bd[1].lo[a] : 0.0;
  }
  if (n > 0 && bd[1].finite > 0) {
    if (!cloud_grid_make(bd[1].lo, bd[1].hi, bd[1].finite, radius, &v.icp_grid)) {
      g_err = "dpe_cloud_icp_stage: radius too small for the cloud's extent";
      return DPE_ERR_ARG;
    }
    HIPC(v.st.ensure(bd[1].finite));
    TRY(cloud_build(c, v.pts[1].p, m, v.icp_grid, 0, v.tcnt, v.st.p));
    // what a step writes
    const size_t blocks = cloud_blocks(n);
    HIPC(v.moved.ensure(3 * n));
    HIPC(v.sq.ensure(n));
    HIPC(v.out.ensure(n));
    HIPC(v.idx.ensure(n));
    HIPC(v.part[0].ensure(blocks * kIcpTerms));
    HIPC(v.part[1].ensure((size_t)cloud_blocks(blocks) * kIcpTerms));
    HIPC(v.matched.ensure(1));
    HIPC(hipStreamSynchronize(c->stream));
  }
  v.icp_staged = true;
  return DPE_OK;
}

// dpe_cloud_icp_step after its prologue.  Timing events: [0] start, [1] apply + build, [2] match, [3] sums,
// [4] download.
int icp_step(DpeContext* c, const double* T, DpeIcpSums* out) {
  CloudScratch& v = c->cloud;
  HIPC(host_wait(c));
  v.timed = false;
  DpeIcpSums s;
  memset(&s, 0, sizeof s);
  const size_t n = v.icp_n;
  if (n == 0 || v.icp_tfinite == 0) { *out = s; return DPE_OK; }   // nothing to match: no launch
  const bool timing = c->pass.timing;
  if (timing) TRY(cloud_events(c));
  IcpXf xf;
  memcpy(xf.m, T, sizeof xf.m);
  IcpOrigins org;
  memcpy(org.s, v.icp_os, sizeof org.s);
  memcpy(org.t, v.icp_ot, sizeof org.t);
  const CloudGrid& g = v.icp_grid;
  if (timing) HIPC(hipEventRecord(v.ev[0], c->stream));
  HIPC(hipMemsetAsync(v.matched.p, 0, sizeof(unsigned long long), c->stream));
  k_icp_apply<<<cloud_blocks(n), kCloudBlock, 0, c->stream>>>(v.pts[0].p, (int)n, xf, v.moved.p);
  HIPC(hipGetLastError());
  g_cloud_launches += 1;
  TRY(cloud_build(c, v.moved.p, n, g, 1, v.qcnt, v.sq.p));
  if (timing) HIPC(hipEventRecord(v.ev[1], c->stream));
  k_cloud_match<<<cloud_blocks(n), kCloudBlock, 0, c->stream>>>(v.sq.p, (int)n, v.st.p, v.tcnt.p, g, v.out.p, v.idx.p);
  HIPC(hipGetLastError());
  if (timing) HIPC(hipEventRecord(v.ev[2], c->stream));
  size_t cnt = cloud_blocks(n);
  k_icp_terms<<<(unsigned)cnt, kCloudBlock, 0, c->stream>>>(v.pts[0].p, (int)n, v.pts[1].p, v.idx.p, v.out.p, org, v.part[0].p,
                                                            v.matched.p);
  HIPC(hipGetLastError());
  g_cloud_launches += 2;
  int at = 0;   // part[at] holds the cnt partials of the level
  while (cnt > 1) {
    const unsigned blocks = cloud_blocks(cnt);
    k_icp_reduce<<<blocks, kCloudBlock, 0, c->stream>>>(v.part[at].p, (int)cnt, v.part[at ^ 1].p);
    HIPC(hipGetLastError());
    g_cloud_launches += 1;
    cnt = blocks;
    at ^= 1;
  }
  if (timing) HIPC(hipEventRecord(v.ev[3], c->stream));
  double sums[kIcpTerms];
  unsigned long long matched = 0;
  HIPC(hipMemcpyAsync(sums, v.part[at].p, sizeof sums, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipMemcpyAsync(&matched, v.matched.p, sizeof matched, hipMemcpyDeviceToHost, c->stream));
  if (timing) HIPC(hipEventRecord(v.ev[4], c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  s.matched = (long long)matched;
  s.d2 = sums[0];
  for (int k = 0; k < 3; ++k) { s.a[k] = sums[1 + k]; s.b[k] = sums[4 + k]; }
  for (int k = 0; k < 9; ++k) s.ab[k] = sums[7 + k];
  *out = s;
  if (timing) {
    for (int e = 0; e < 4; ++e) HIPC(hipEventElapsedTime(&v.ms[e], v.ev[e], v.ev[e + 1]));
    v.timed = true;
  }
  return DPE_OK;
}

unsigned render_blocks(size_t n) { return (unsigned)((n + kRenderBlock - 1) / kRenderBlock); }

// dpe_cloud_render_stage after its prologue: the scan resident in pts[0].  Timing events: [0] start, [1] staged.
int render_stage(DpeContext* c, const float* xyz, size_t n) {
  CloudScratch& v = c->cloud;
  HIPC(host_wait(c));
  const bool timing = c->pass.timing;
  v.timed = false;
  v.icp_staged = false;
  v.render_staged = false;
  if (timing) TRY(cloud_events(c));
  if (timing) HIPC(hipEventRecord(v.ev[0], c->stream));
  if (n > 0) {
    HIPC(v.pts[0].ensure(3 * n));
    HIPC(hipMemcpyAsync(v.pts[0].p, xyz, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  }
  if (timing) HIPC(hipEventRecord(v.ev[1], c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  v.render_n = n;
  v.render_staged = true;
  if (timing) {
    for (float& t : v.ms) t = 0.f;
    HIPC(hipEventElapsedTime(&v.ms[0], v.ev[0], v.ev[1]));
    v.timed = true;
  }
  return DPE_OK;
}

// dpe_cloud_render_view after its prologue.  Timing events: [0] start, [1] rendered, [2] downloaded.
int render_view(DpeContext* c, const DpeCamera& cam, int splat, float* depth_out) {
  CloudScratch& v = c->cloud;
  HIPC(host_wait(c));
  const bool timing = c->pass.timing;
  v.timed = false;
  if (timing) TRY(cloud_events(c));
  const size_t npx = (size_t)cam.width * (size_t)cam.height, n = v.render_n;
  v.rmap_w = v.rmap_h = 0;   // the old map goes with the first launch
  HIPC(v.rmap.ensure(npx));
  if (timing) HIPC(hipEventRecord(v.ev[0], c->stream));
  k_render_clear<<<render_blocks(npx), kRenderBlock, 0, c->stream>>>(v.rmap.p, npx);
  HIPC(hipGetLastError());
  if (n > 0) {
    k_render_splat<<<render_blocks(n), kRenderBlock, 0, c->stream>>>(v.pts[0].p, (int)n, cam, splat, v.rmap.p);
    HIPC(hipGetLastError());
    g_cloud_launches += 1;
  }
  k_render_finish<<<render_blocks(npx), kRenderBlock, 0, c->stream>>>(v.rmap.p, npx);
  HIPC(hipGetLastError());
  g_cloud_launches += 2;
  if (timing) HIPC(hipEventRecord(v.ev[1], c->stream));
  if (depth_out) HIPC(hipMemcpyAsync(depth_out, v.rmap.p, npx * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (timing) HIPC(hipEventRecord(v.ev[2], c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  v.rmap_w = cam.width;
  v.rmap_h = cam.height;
  if (timing) {
    for (float& t : v.ms) t = 0.f;
    HIPC(hipEventElapsedTime(&v.ms[1], v.ev[0], v.ev[1]));
    HIPC(hipEventElapsedTime(&v.ms[3], v.ev[1], v.ev[2]));
    v.timed = true;
  }
  return DPE_OK;
}

// dpe_depth_score after its prologue; gt == nullptr: against the resident map.  Timing events: [0] start,
// [1] uploaded, [2] scored, [3] downloaded.
int depth_score(DpeContext* c, const float* est, const float* gt, int w, int h, const DepthTaus& T, DpeDepthScore* out,
                float* err) {
  CloudScratch& v = c->cloud;
  HIPC(host_wait(c));
  const bool timing = c->pass.timing;
  v.timed = false;
  if (timing) TRY(cloud_events(c));
  const size_t npx = (size_t)w * (size_t)h;
  size_t cnt = render_blocks(npx);
  HIPC(v.s_est.ensure(npx));
  if (gt) HIPC(v.s_gt.ensure(npx));
  if (err) HIPC(v.s_err.ensure(npx));
  HIPC(v.s_part[0].ensure(cnt * kDepthTerms));
  HIPC(v.s_part[1].ensure((size_t)render_blocks(cnt) * kDepthTerms));
  HIPC(v.s_cnt.ensure(kDepthCounters));
  if (timing) HIPC(hipEventRecord(v.ev[0], c->stream));
  HIPC(hipMemcpyAsync(v.s_est.p, est, npx * sizeof(float), hipMemcpyHostToDevice, c->stream));
  if (gt) HIPC(hipMemcpyAsync(v.s_gt.p, gt, npx * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPC(hipMemsetAsync(v.s_cnt.p, 0, kDepthCounters * sizeof(unsigned long long), c->stream));
  if (timing) HIPC(hipEventRecord(v.ev[1], c->stream));
  const float* g = gt ? v.s_gt.p : reinterpret_cast<const float*>(v.rmap.p);
  k_depth_score<<<(unsigned)cnt, kRenderBlock, 0, c->stream>>>(v.s_est.p, g, npx, T, v.s_part[0].p, v.s_cnt.p,
                                                               err ? v.s_err.p : nullptr);
  HIPC(hipGetLastError());
  g_cloud_launches += 1;
  int at = 0;   // s_part[at] holds the cnt partials of the level
  while (cnt > 1) {
    const unsigned blocks = render_blocks(cnt);
    k_depth_reduce<<<blocks, kRenderBlock, 0, c->stream>>>(v.s_part[at].p, cnt, v.s_part[at ^ 1].p);
    HIPC(hipGetLastError());
    g_cloud_launches += 1;
    cnt = blocks;
    at ^= 1;
  }
  if (timing) HIPC(hipEventRecord(v.ev[2], c->stream));
  double sums[kDepthTerms];
  unsigned long long counts[kDepthCounters];
  HIPC(hipMemcpyAsync(sums, v.s_part[at].p, sizeof sums, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipMemcpyAsync(counts, v.s_cnt.p, sizeof counts, hipMemcpyDeviceToHost, c->stream));
  if (err) HIPC(hipMemcpyAsync(err, v.s_err.p, npx * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (timing) HIPC(hipEventRecord(v.ev[3], c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  DpeDepthScore s;
  memset(&s, 0, sizeof s);
  s.n_px = (long long)npx;
  s.n_gt = (long long)counts[0];
  s.n_est = (long long)counts[1];
  s.n_both = (long long)counts[2];
  for (int k = 0; k < T.n; ++k) s.within[k] = (long long)counts[3 + k];
  s.sum_abs = sums[0];
  s.sum_rel = sums[1];
  s.sum_sq = sums[2];
  *out = s;
  if (timing) {
    for (float& t : v.ms) t = 0.f;
    HIPC(hipEventElapsedTime(&v.ms[0], v.ev[0], v.ev[1]));
    HIPC(hipEventElapsedTime(&v.ms[2], v.ev[1], v.ev[2]));
    HIPC(hipEventElapsedTime(&v.ms[3], v.ev[2], v.ev[3]));
    v.timed = true;
  }
  return DPE_OK;
}

}  // namespace

extern "C" int dpe_cloud_render_stage(DpeContext* c, const float* xyz, size_t n) {
  TRY(enter(c, n <= (size_t)INT_MAX && (xyz || n == 0), "dpe_cloud_render_stage: bad argument"));
  return render_stage(c, xyz, n);
}

extern "C" int dpe_cloud_render_view(DpeContext* c, const DpeCamera* cam, int splat, float* depth_out) {
  const bool ok = cam && cam->width >= 1 && cam->height >= 1 && splat >= 0 && splat <= DPE_DEPTH_MAX_SPLAT;
  TRY(enter(c, ok, "dpe_cloud_render_view: bad argument"));
  if (!c->cloud.render_staged) {
    g_err = "dpe_cloud_render_view: no staged cloud (dpe_cloud_render_stage comes first)";
    return DPE_ERR_STATE;
  }
  return render_view(c, *cam, splat, depth_out);
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
  if (!gt) {
    if (c->cloud.rmap_w == 0) {
      g_err = "dpe_depth_score: no rendered map (dpe_cloud_render_view comes first, or pass gt)";
      return DPE_ERR_STATE;
    }
    if (c->cloud.rmap_w != w || c->cloud.rmap_h != h) {
      g_err = "dpe_depth_score: the size differs from the rendered map's";
      return DPE_ERR_ARG;
    }
  }
  return depth_score(c, est, gt, w, h, T, out, err);
}

extern "C" int dpe_cloud_nn_index(DpeContext* c, const float* query, size_t n, const float* target, size_t m, float radius,
                                  float* d2_out, int32_t* idx_out) {
  const bool ok = cloud_args_ok(query, n, target, m, radius, d2_out, nullptr, false) && (idx_out || n == 0);
  TRY(enter(c, ok, "dpe_cloud_nn_index: bad argument"));
  int32_t none = -1;   // n == 0: no entry, and the call still stages as one with indices
  return cloud_run(c, query, n, target, m, radius, d2_out, idx_out ? idx_out : &none, nullptr, "dpe_cloud_nn_index");
}

extern "C" int dpe_cloud_icp_stage(DpeContext* c, const float* src, size_t n, const float* tgt, size_t m, float radius) {
  const bool ok = n <= (size_t)INT_MAX && m <= (size_t)INT_MAX && (src || n == 0) && (tgt || m == 0) && std::isfinite(radius) &&
                  radius > 0.0f;
  TRY(enter(c, ok, "dpe_cloud_icp_stage: bad argument"));
  return icp_stage(c, src, n, tgt, m, radius);
}

extern "C" int dpe_cloud_icp_step(DpeContext* c, const double* T, DpeIcpSums* out) {
  TRY(enter(c, T && out, "dpe_cloud_icp_step: bad argument"));
  if (!c->cloud.icp_staged) {
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
  if (!c || !ms || !c->cloud.timed) return 0;
  int k = 0;
  for (; k < n && k < 4; ++k) ms[k] = c->cloud.ms[k];
  return k;
}
