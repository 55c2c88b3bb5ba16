// dpe_cloud.hip -- the cloud evaluation's distances (dpe_cloud_nn, dpe_cloud_nn_pair) and the voxel
// down-sampling (dpe_cloud_voxel) of include/dpe_mvs.h: the kernels of pass_cloud.h and pass_voxel.h over the
// context's cloud scratch.  A unit of libdpe_mvs.so; the concurrency
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
// ev: the three timing events of this direction (end of build, query, download), or null.
int cloud_direction(DpeContext* c, int qi, size_t n, int ti, size_t m, const CloudBounds& tb, float radius, float* out,
                    Event* ev, const char* who) {
  if (n == 0) return DPE_OK;
  CloudScratch& v = c->cloud;
  if (tb.finite == 0) {   // nothing to find: no launch
    const float r2 = radius * radius;
    for (size_t i = 0; i < n; ++i) out[i] = r2;
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
  TRY(cloud_build(c, v.pts[ti].p, m, g, 0, v.tcnt, v.st.p));
  TRY(cloud_build(c, v.pts[qi].p, n, g, 1, v.qcnt, v.sq.p));
  if (ev) HIPC(hipEventRecord(ev[0], c->stream));
  k_cloud_query<<<cloud_blocks(n), kCloudBlock, 0, c->stream>>>(v.sq.p, (int)n, v.st.p, v.tcnt.p, g, v.out.p);
  HIPC(hipGetLastError());
  g_cloud_launches += 1;
  if (ev) HIPC(hipEventRecord(ev[1], c->stream));
  HIPC(hipMemcpyAsync(out, v.out.p, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (ev) HIPC(hipEventRecord(ev[2], c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  return DPE_OK;
}

bool cloud_args_ok(const float* a, size_t n, const float* b, size_t m, float radius, const float* a_out, const float* b_out,
                   bool need_b_out) {
  return n <= (size_t)INT_MAX && m <= (size_t)INT_MAX && (a || n == 0) && (b || m == 0) && (a_out || n == 0) &&
         (!need_b_out || b_out || m == 0) && std::isfinite(radius) && radius > 0.0f;
}

// the two clouds staged once; a_to_b always, b_to_a when it is not null
int cloud_run(DpeContext* c, const float* a, size_t n, const float* b, size_t m, float radius, float* a_to_b, float* b_to_a,
              const char* who) {
  CloudScratch& v = c->cloud;
  HIPC(host_wait(c));
  const bool timing = c->pass.timing;
  v.timed = false;
  if (timing && v.ev.empty()) {
    for (int k = 0; k < 8; ++k) {
      Event e;
      HIPC(e.create(hipEventDefault));
      v.ev.push_back(std::move(e));
    }
  }
  if (timing) HIPC(hipEventRecord(v.ev[0], c->stream));
  TRY(cloud_stage(c, 0, a, n));
  TRY(cloud_stage(c, 1, b, m));
  if (timing) HIPC(hipEventRecord(v.ev[1], c->stream));
  uint32_t raw[16];
  HIPC(hipMemcpyAsync(raw, v.bounds.p, sizeof raw, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  CloudBounds bd[2];
  for (int w = 0; w < 2; ++w) {
    bd[w].finite = raw[8 * w + 6];
    for (int k = 0; k < 3; ++k) { bd[w].lo[k] = cloud_unkey(~raw[8 * w + k]); bd[w].hi[k] = cloud_unkey(raw[8 * w + 3 + k]); }
  }
  TRY(cloud_direction(c, 0, n, 1, m, bd[1], radius, a_to_b, timing ? &v.ev[2] : nullptr, who));
  if (b_to_a) TRY(cloud_direction(c, 1, m, 0, n, bd[0], radius, b_to_a, timing ? &v.ev[5] : nullptr, who));
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
  if (timing && v.ev.empty()) {
    for (int e = 0; e < 8; ++e) {
      Event ev;
      HIPC(ev.create(hipEventDefault));
      v.ev.push_back(std::move(ev));
    }
  }
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

}  // namespace

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
  return cloud_run(c, query, n, target, m, radius, d2_out, nullptr, "dpe_cloud_nn");
}

extern "C" int dpe_cloud_nn_pair(DpeContext* c, const float* a, size_t n, const float* b, size_t m, float radius,
                                 float* a_to_b, float* b_to_a) {
  TRY(enter(c, cloud_args_ok(a, n, b, m, radius, a_to_b, b_to_a, true), "dpe_cloud_nn_pair: bad argument"));
  float none = 0.f;   // m == 0: b_to_a has no entry, and the second direction still runs as one
  return cloud_run(c, a, n, b, m, radius, a_to_b, b_to_a ? b_to_a : &none, "dpe_cloud_nn_pair");
}

extern "C" int dpe_cloud_last_timings(DpeContext* c, float* ms, int n) {
  if (!c || !ms || !c->cloud.timed) return 0;
  int k = 0;
  for (; k < n && k < 4; ++k) ms[k] = c->cloud.ms[k];
  return k;
}
