// pass_neighbours.h — the neighbour subsystem of a pass: GenNeighbours (DPE.cu:2103-2463) in its two
// kernels, NeigbourUpdate and RANSACToGetFitPlane.
//
// The steps that GenNeighbours and the fit share are stated once, at the top: the edge-limit draw,
// the probe batch, the label extension, the triple draw, the normal-agreement test, the plane
// through three points, a plane's depth at a pixel and the centre cost.  GenNeighbours' collection
// phase (the direction walks, then the label extension) is one function over the caller's store;
// its fit loop is written twice, because the two kernels differ exactly where the fit needs an
// order: the scratch kernel keeps the reference's insertion sorts, whose behaviour under NaN is
// the reference's, and the scratch-free kernel replaces them by selections that hold only without
// NaN and defers a pixel to the scratch kernel otherwise.
#pragma once
#include "pass_kernels.h"   // PIX2D_FULL

namespace dpe {

// ------------------------------------------------------------------------------ shared steps
constexpr int kGnSpec = 4;     // probe attempts drawn and loaded together
constexpr int kGnMargin = 6;   // support points keep this far from the border (min_margin)

// The use_limit / use_edge draw (DPE.cu:2141-2152, :2921-2930): whether edges limit this pixel,
// and the complex_ value GenNeighbours then stores (< 0: none).  The store is the caller's.
struct GnLimit { bool edge_limit; float complex_new; };
DEV GnLimit gn_limit_draw(const PassConst& pc, const DevBufs& B, int center, Rng& rs) {
  GnLimit r{false, -1.0f};
  if (pc.P.use_limit) {
    r.edge_limit = true;
    if (pc.P.use_edge) {
      const float cv = B.complex_[center];
      const float rp = rng_uniform(rs) - 1.1920929e-07f;
      if (rp < cv) r.edge_limit = false;
      else r.complex_new = MAXo(0.99f, cv);
    }
  }
  return r;
}

// the angle test of a probe, td = normalize(np - p), td . od > thr (DPE.cu:2196-2199)
DEV bool gn_angle_ok(float dxf, float dyf, float2 od, float thr) {
  float2 td = make_float2(dxf, dyf);
  normalize2(td);
  return td.x * od.x + td.y * od.y > thr;
}

// The probes of direction `od` at one radius (DPE.cu:2170-2210), kGnSpec attempts at a time:
// their draws, targets and weak[] / nearest[] loads are all issued first, then the attempts are
// tested in order; the stream is then positioned just after the attempt that succeeded (each
// attempt draws 4 words; the stream is position-addressable), so the draws consumed are the
// serial loop's.  `blocked(np)` is the caller's walk test between the pixel and np; the point found
// goes to the caller's push(np).
template <class Push, class Blocked>
DEV bool gn_probe_batch(const PassConst& pc, const DevBufs& B, Rng& rs, int x, int y, int center, float2 od,
                        int radius, bool edge_limit, Push push, Blocked blocked) {
  const int W = pc.W, H = pc.H;
  const int shift_range = pc.gn_shift;
  bool found = false;
  for (int ra = 0; ra < 4 && !found; ra += kGnSpec) {
    short2 cand[kGnSpec], nnv[kGnSpec];
    uint8_t wkv[kGnSpec];
    bool inm[kGnSpec];
    const uint32_t pos0 = rs.idx == 4 ? rs.ctr * 4u : (rs.ctr - 1u) * 4u + (uint32_t)rs.idx;
#pragma unroll
    for (int q = 0; q < kGnSpec; ++q) {
      const uint32_t r1 = rng_u32(rs); const uint32_t r2 = rng_u32(rs);
      const uint32_t r3 = rng_u32(rs); const uint32_t r4 = rng_u32(rs);
      const int rxs = (int)(((r1 % 2 == 0) ? 1u : 0xFFFFFFFFu) * r2 % (uint32_t)shift_range);
      const int rys = (int)(((r3 % 2 == 0) ? 1u : 0xFFFFFFFFu) * r4 % (uint32_t)shift_range);
      float2 dir = make_float2(od.x * 20 + (float)rxs, od.y * 20 + (float)rys);
      normalize2(dir);
      const short2 np = make_short2((short)f2i((float)x + dir.x * radius), (short)f2i((float)y + dir.y * radius));
      inm[q] = !(np.x < kGnMargin || np.y < kGnMargin || np.x >= W - kGnMargin || np.y >= H - kGnMargin);
      const int npc = inm[q] ? np.x + np.y * W : center;
      wkv[q] = B.weak[npc];
      nnv[q] = B.nearest[npc];
      cand[q] = np;
    }
#pragma unroll
    for (int q = 0; q < kGnSpec; ++q) {
      if (found || !inm[q]) continue;
      short2 np = cand[q];
      if (wkv[q] != DPE_STRONG) {
        np = nnv[q];
        if (np.x == -1 || np.y == -1) continue;
      }
      if (gn_angle_ok((float)(np.x - x), (float)(np.y - y), od, pc.gn_thr) && (!edge_limit || !blocked(np))) {
        push(np);
        found = true;
        rng_seek(rs, pos0 + 4u * (uint32_t)(q + 1));
      }
    }
  }
  return found;
}

// The label extension (DPE.cu:2213-2279): along each of the 8 directions to the pixel's label
// boundary, 2 * rotate_time - 1 evenly spaced points on the even directions and one on the odd
// (dir_step, :2236-2247), each replaced by its nearest strong pixel where it is not strong itself.
template <class Push>
DEV void gn_extend_labels(const PassConst& pc, const DevBufs& B, int x, int y, int center, Push push) {
  const int W = pc.W, H = pc.H;
  if (!(pc.P.use_label && B.label[center] > 0)) return;
  const short2* lb = B.lab_bound + (size_t)center * 8;
#pragma unroll 1   // one copy of the f64 square root and division, not eight
  for (int i = 0; i < 8; ++i) {
    const short2 bp = lb[i];
    float dist = 0.0f;
    if (bp.x != -1 && bp.y != -1) {
      const double dxx = (double)(x - bp.x), dyy = (double)(y - bp.y);
      dist = (float)__builtin_sqrt(dxx * dxx + dyy * dyy);
      if (i >= 4) dist = (float)((double)dist / 1.4142135623730951);
    }
    const int nstep = (i % 2 == 0) ? 2 * pc.P.rotate_time - 1 : 1;
    const int step_len = MAXo(1, d2i(__builtin_floor(1.0 * dist / (nstep + 1))));
    for (int step = 1; step <= nstep; ++step) {
      short2 np = make_short2((short)(x + step * step_len * kDir[i][0]), (short)(y + step * step_len * kDir[i][1]));
      if (np.x < kGnMargin || np.y < kGnMargin || np.x >= W - kGnMargin || np.y >= H - kGnMargin) continue;
      int npc = np.x + np.y * W;
      if (B.weak[npc] != DPE_STRONG) {
        np = B.nearest[npc];
        if (np.x == -1 || np.y == -1) continue;
        npc = np.x + np.y * W;
      }
      if (B.label[npc] != 0 && B.label[npc] != B.label[center]) continue;
      push(np);
    }
  }
}

// GenNeighbours' collection phase: every support point of the pixel goes to push(np), in the order
// of the reference's compaction of strong_points[] (dir_index grows through the probe loops, the
// label extension follows at 32+; rotate_time <= 4, refused otherwise by stage_check_args).
// The 8 x rotate_time direction walks are ONE loop per lane: a lane that ends a walk (support point
// found, radius past the image or 4096) moves on to its next direction at once, so a wave's time
// is its slowest lane's total walk, not the sum over directions of each direction's slowest walk.
// Each lane's sequence of probes (and of Philox draws) is the nested loops' sequence.
// note(k) is the caller's diagnostics: kGnNoteStep at every radius step, kGnNoteWalked between the
// walks and the extension.
enum { kGnNoteStep = 0, kGnNoteWalked = 1 };
template <class Push, class Blocked, class Note>
DEV void gn_collect(const PassConst& pc, const DevBufs& B, Rng& rs, int x, int y, int center, bool edge_limit,
                    Push push, Blocked blocked, Note note) {
  const int W = pc.W, H = pc.H;
  const int rotate_time = pc.P.rotate_time;
  const float cos_angle = pc.gn_cos, sin_angle = pc.gn_sin;
  auto origin_od = [](int oi) -> float2 {   // odx -1..1 outer, ody -1..1 inner, (0, 0) skipped
    const int k = oi < 4 ? oi : oi + 1;
    float2 od = make_float2((float)(k / 3 - 1), (float)(k % 3 - 1));
    normalize2(od);
    return od;
  };
  int oi = 0, ri = 0, radius = 2;
  float2 od = origin_od(0);
  while (oi < 8) {
    bool next = radius > 4096;
    note(kGnNoteStep);
    if (!next) {
      const float tpx = (float)x + od.x * radius, tpy = (float)y + od.y * radius;
      if (tpx < 0 || tpy < 0 || tpx >= W || tpy >= H) next = true;
    }
    if (!next) {
      if (gn_probe_batch(pc, B, rs, x, y, center, od, radius, edge_limit, push, blocked)) next = true;
      else radius = MINo(radius * 2, radius + 25);
    }
    if (next) {
      radius = 2;
      if (++ri < rotate_time) {
        float2 rd = make_float2(od.x * cos_angle - od.y * sin_angle, od.x * sin_angle + od.y * cos_angle);
        normalize2(rd);
        od = rd;
      } else {
        ri = 0;
        if (++oi < 8) od = origin_od(oi);
      }
    }
  }
  note(kGnNoteWalked);
  gn_extend_labels(pc, B, x, y, center, push);
}

// three indices below n from the stream; false when two of them coincide
DEV bool gn_draw_triple(Rng& rs, int n, int& a, int& b, int& c) {
  a = (int)(rng_u32(rs) % (uint32_t)n);
  b = (int)(rng_u32(rs) % (uint32_t)n);
  c = (int)(rng_u32(rs) % (uint32_t)n);
  return !(a == b || b == c || a == c);
}
// the three normals lie within 30 degrees of one another (V: float3 or float4, xyz the normal)
template <class V>
DEV bool gn_normals_agree(const V& AN, const V& BN, const V& CN) {
  return !((double)(AN.x * BN.x + AN.y * BN.y + AN.z * BN.z) < 0.8660254 ||
           (double)(AN.x * CN.x + AN.y * CN.y + AN.z * CN.z) < 0.8660254 ||
           (double)(BN.x * CN.x + BN.y * CN.y + BN.z * CN.z) < 0.8660254);
}
// the plane through A, B, C (unit normal, w = -n . A); ok is false, and the result not a plane, when
// their cross product is zero or NaN.  Returned by value: as an out-parameter the fit kernel took one
// VGPR more
DEV float4 gn_plane3(const float3 A, const float3 Bq, const float3 C, bool& ok) {
  float4 cv; ok = false;
  const float ACx = A.x - C.x, ACy = A.y - C.y, ACz = A.z - C.z;
  const float BCx = Bq.x - C.x, BCy = Bq.y - C.y, BCz = Bq.z - C.z;
  cv.x = ACy * BCz - BCy * ACz;
  cv.y = -(ACx * BCz - BCx * ACz);
  cv.z = ACx * BCy - BCx * ACy;
  if ((cv.x == 0 && cv.y == 0 && cv.z == 0) || cv.x != cv.x || cv.y != cv.y || cv.z != cv.z) return cv;
  normalize3(cv);
  cv.w = -(cv.x * A.x + cv.y * A.y + cv.z * A.z);
  ok = true;
  return cv;
}
// depth of plane pl at the normalised image coordinates (fx, fy)
DEV float gn_plane_depth(const float4& pl, float fx, float fy) { return -pl.w / (pl.x * fx + pl.y * fy + pl.z); }
// how far plane cv passes from the pixel's own depth cpz (DPE.cu:2352-2356)
DEV float gn_centre_cost(const DpeCamera& camera, const float4& cv, int x, int y, float cpz) {
  const float fx = ((float)x - camera.K[2]) / camera.K[0];
  const float fy = ((float)y - camera.K[5]) / camera.K[4];
  return __builtin_fabsf(gn_plane_depth(cv, fx, fy) - cpz);
}

// ------------------------------------------------------------------------------ GenNeighbours, scratch kernel
// One WEAK pixel of GenNeighbours with per-thread arrays in scratch: the fallback for the pixels
// k_gen_neighbours_lds defers (more support points than its LDS slots, or a NaN where its
// selections need an order).  Its store holds the 64 points a pixel can collect at rotate_time <= 4
// (stage_check_args refuses any other).  The fit keeps the reference's insertion sorts, its
// zero-initialised residuals[DPE_NEIGHBOUR_NUM] and its cache of edge tests.
DEV void gen_neighbours_px(const PassConst& pc, const DevBufs& B, int center) {   // DPE.cu:2103-2463
  const int W = pc.W;
  PHASE_BEGIN();
  const int x = center % W, y = center / W;
  const float depth_diff = pc.P.depth_max - pc.P.depth_min;
  const DpeCamera& camera = pc.cams[0];
  Rng rs; rng_init(rs, (uint32_t)center, pc.seed32, STREAM_GEN_NEIGHBOURS, pc.salt);
  short2* nb = B.nb + (size_t)center * 9;
  nb[0] = make_short2((short)x, (short)y);
  for (int i = 1; i < 9; ++i) nb[i] = make_short2(-1, -1);
  const float ransac_threshold = pc.P.ransac_threshold * depth_diff;
  const GnLimit lim = gn_limit_draw(pc, B, center, rs);
  const bool edge_limit = lim.edge_limit;
  if (lim.complex_new >= 0.0f) B.complex_[center] = lim.complex_new;   // at once: nothing defers this pixel
  short2 spv[64];
  int valid_count = 0;
  gn_collect(pc, B, rs, x, y, center, edge_limit,
             [&](short2 np) { spv[valid_count++] = np; },
             [&](short2 np) -> bool { return bresenham(pc, B, x, y, np.x, np.y); },
             [&](int k) { if (k == kGnNoteWalked) PHASE(0); });
  PHASE(1);
  if (valid_count <= 3) { B.weak_rel[center] = 0; PHASE_END_ALL(2); return; }

  // per point only the depth is kept: its 3-D point and normal are recomputed from (pixel, depth) /
  // planes[] when a, b, c are drawn (same expressions, same bits), which halves the per-thread scratch.
  float spd[64];
  float X[3];
  get3d(camera, x, y, B.planes0[center].w, X);
  const float cpz = X[2];
  for (int i = 0; i < valid_count; ++i) spd[i] = B.planes0[spv[i].x + spv[i].y * W].w;
  for (int i = valid_count; i < 64; ++i) spv[i] = make_short2(-1, -1);
  // normalised image coordinates of each support point: loop-invariant in the RANSAC iterations
  // below (same expression, same bits as evaluating it per iteration)
  float2 spf[64];
  for (int i = 0; i < valid_count; ++i)
    spf[i] = make_float2(((float)spv[i].x - camera.K[2]) / camera.K[0], ((float)spv[i].y - camera.K[5]) / camera.K[4]);
  auto point3 = [&](int i) -> float3 {
    float Y[3];
    get3d(camera, spv[i].x, spv[i].y, spd[i], Y);
    return make_float3(Y[0], Y[1], Y[2]);
  };
  auto normal3 = [&](int i) -> float4 { return transform_normal_ref(camera, B.planes0[spv[i].x + spv[i].y * W]); };
  PHASE(2);
  float4 best_plane = make_float4(0, 0, 0, 0);
  bool has_valid_plane = false;
  {
    int iteration = 50, max_iter = pc.P.high_res_img ? 200 : 125, max_count = 3;
    // residuals[i < valid_count] are written before every read; of the rest only index
    // DPE_NEIGHBOUR_NUM is ever read (as the reference's zero-initialised entry)
    float min_cost = 3.40282347e+38f, residuals[64];
    for (int i = valid_count; i <= DPE_NEIGHBOUR_NUM; ++i) residuals[i] = 0.0f;
    float temp_thr = ransac_threshold;
    // edge_test[64][64] (DPE.cu:2307) as two bit matrices: tested / crosses-an-edge
    // rows are zeroed on first use (row_live), not up front: a thread touches a few of the 64
    uint64_t tested[64], crosses[64], row_live = 0;
    bool has_consist_normal_plane = false;
    bool must_in_triangle = (pc.P.use_label && B.label[center] > 0 && edge_limit) ? false : true;
    auto edge_pair = [&](int a, int b) -> bool {   // returns edge_test[a][b] == 1
      if (!((row_live >> a) & 1ull)) { tested[a] = 0; crosses[a] = 0; row_live |= 1ull << a; }
      if (!((row_live >> b) & 1ull)) { tested[b] = 0; crosses[b] = 0; row_live |= 1ull << b; }
      if (!((tested[a] >> b) & 1ull)) {
        const bool c = bresenham(pc, B, spv[a].x, spv[a].y, spv[b].x, spv[b].y);
        tested[a] |= 1ull << b; tested[b] |= 1ull << a;
        if (c) { crosses[a] |= 1ull << b; crosses[b] |= 1ull << a; }
      }
      return (crosses[a] >> b) & 1ull;
    };
    while (iteration > 0 && max_iter > 0) {
      max_iter--;
      int a, b, c;
      if (!gn_draw_triple(rs, valid_count, a, b, c)) continue;
      if (must_in_triangle && !point_in_triangle(spv[a], spv[b], spv[c], x, y)) continue;
      if (edge_limit) {
        const bool eab = edge_pair(a, b);
        const bool ebc = edge_pair(b, c);
        const bool eca = edge_pair(c, a);
        if (eab || ebc || eca) continue;
      }
      bool normal_consistency = false;
      if (pc.P.geom_consistency && edge_limit) {
        normal_consistency = gn_normals_agree(normal3(a), normal3(b), normal3(c));
        if (has_consist_normal_plane && !normal_consistency) continue;
      }
      iteration--;
      bool ok;
      const float4 cv = gn_plane3(point3(a), point3(b), point3(c), ok);
      if (!ok) continue;
      // residual of support point si under cv (stored only when a new best plane needs the sort)
      auto resid = [&](int si) -> float { return __builtin_fabsf(gn_plane_depth(cv, spf[si].x, spf[si].y) - spd[si]); };
      int temp_count = 0;
      for (int si = 0; si < valid_count; ++si)
        if (resid(si) < temp_thr) temp_count++;
      if (temp_count < 6) continue;
      if (temp_count > max_count) {
        if (!must_in_triangle && point_in_triangle(spv[a], spv[b], spv[c], x, y)) must_in_triangle = true;
        if (!has_consist_normal_plane && normal_consistency) has_consist_normal_plane = true;
        const float cd = gn_centre_cost(camera, cv, x, y, cpz);
        best_plane = cv; max_count = temp_count; min_cost = cd; has_valid_plane = true;
        if ((double)temp_thr > (pc.P.high_res_img ? 0.05 : 0.005)) {
          for (int si = 0; si < valid_count; ++si) residuals[si] = resid(si);
          // sort_small(residuals, valid_count) (DPE.cu:5-14)
          for (int i = 1; i < valid_count; i++) {
            const float tmp = residuals[i];
            int j = i;
            for (; j >= 1 && tmp < residuals[j - 1]; j--) residuals[j] = residuals[j - 1];
            residuals[j] = tmp;
          }
          if (temp_thr < residuals[DPE_NEIGHBOUR_NUM]) continue;
          temp_thr = (float)((double)residuals[DPE_NEIGHBOUR_NUM] - 1e-6);
          temp_count = 0;
          for (int i = 0; i < valid_count; ++i) {
            if (residuals[i] < temp_thr) temp_count++;
            else break;
          }
          max_count = temp_count;
        }
      } else if (temp_count == max_count) {
        if (!must_in_triangle && point_in_triangle(spv[a], spv[b], spv[c], x, y)) must_in_triangle = true;
        const float cd = gn_centre_cost(camera, cv, x, y, cpz);
        if (cd < min_cost) { best_plane = cv; max_count = temp_count; min_cost = cd; }
      }
    }
  }
  PHASE(3);
  if (!has_valid_plane) { B.weak_rel[center] = 0; PHASE_END_ALL(2); return; }
  float* weight = spd;          // in place: weight[i] is written after spd[i] is read
  for (int i = 0; i < valid_count; ++i) {
    const float dist = __builtin_fabsf(gn_plane_depth(best_plane, spf[i].x, spf[i].y) - spd[i]);
    if (dist >= ransac_threshold) { spv[i] = make_short2(-1, -1); weight[i] = 3.40282347e+38f; continue; }
    weight[i] = dist;
  }
  // sort_small_weighted (DPE.cu:16-29)
  for (int i = 1; i < valid_count; i++) {
    const short2 tp = spv[i]; const float tw = weight[i];
    int j = i;
    for (; j >= 1 && tw < weight[j - 1]; j--) { spv[j] = spv[j - 1]; weight[j] = weight[j - 1]; }
    spv[j] = tp; weight[j] = tw;
  }
  for (int i = 1; i < DPE_NEIGHBOUR_NUM; ++i) nb[i] = spv[i - 1];
  B.weak_rel[center] = 1;
  PHASE(4);
  PHASE_END_ALL(2);
}
// over `list`: a small persistent grid (kGnOvfBlocks x 256 threads) striding through the list, so
// that the usual empty overflow list costs one short launch (the round-4 full-grid launch took the
// aux stream for 0.7 ms)
constexpr int kGnOvfBlocks = 64;
__global__ void __launch_bounds__(256) k_gen_neighbours(const PassConst* __restrict__ pcp, DevBufs B,
                                                        const int* __restrict__ list, const int* __restrict__ nlist_p) {
  const PassConst& pc = *pcp;
  const int n = *nlist_p;
  for (int gi = blockIdx.x * blockDim.x + threadIdx.x; gi < n; gi += gridDim.x * blockDim.x)
    gen_neighbours_px(pc, B, list[gi]);
}

// ------------------------------------------------------------------------------ GenNeighbours, scratch-free
// The same GenNeighbours with no per-thread arrays (k_gen_neighbours keeps them in scratch, re-read
// from HBM on every RANSAC try).  The collection phase appends the support points in the order of
// the reference's compaction, so they go straight into an LDS column per thread: the packed pixel,
// K slots ([slot][thread], conflict-free; K = 16 x rotate_time rounded up to 32 / 64 holds the most
// a pixel can collect: 8 KB / 16 KB per 64-thread workgroup).  A point's depth is re-read from
// planes0[] and its normalised image coordinates come from per-column / per-row tables (`gtab`, the
// same expression per coordinate), so nothing else is stored.  The edge tests are recomputed instead
// of cached (BresenhamLine is a pure function of its end points; the reference's edge_test[][] only
// saves work), and the two sorts become order-statistic selections whose results equal the
// insertion sorts' whenever no residual or weight is NaN.  A pixel with more than K support points,
// or a NaN where a sort needs the order, writes nothing and is appended to `ovf` for
// k_gen_neighbours (its Philox stream is addressed by the pixel, so the rerun draws the same
// numbers).  90 VGPRs, no scratch; 5 waves per SIMD at K = 8 / 32, 3 at K = 64 (by its LDS).
constexpr int kGnBT = 64;   // threads per workgroup
// table of the normalised image coordinates: gtab[x] = (x - K[2]) / K[0], gtab[W + y] = (y - K[5]) / K[4]
__global__ void k_gn_tables(const PassConst* __restrict__ pcp, float* __restrict__ gtab) {
  const PassConst& pc = *pcp;
  const DpeCamera& camera = pc.cams[0];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < pc.W) gtab[i] = ((float)i - camera.K[2]) / camera.K[0];
  else if (i < pc.W + pc.H) gtab[i] = ((float)(i - pc.W) - camera.K[5]) / camera.K[4];
}
// Per-pixel durations of the scratch-free GenNeighbours (DPE_DIAG & 8; tools/gn_times.py): shader
// clocks from the start to the end of the probes and to the pixel's end, at the pixel's list index
// (one wave = 64 consecutive indices).  Off in the product.
#if DPE_GN_TIMES
// + per-pixel counts: [0] radius steps of the direction walks, [1] Bresenham walks of the probes,
// [2] RANSAC tries, [3] Bresenham walks of the RANSAC, [4] / [5] shader clocks in the probes' / the
// RANSAC's Bresenham walks
static __device__ uint32_t g_gntime[2 << 20];
static __device__ uint32_t g_gncnt[6 << 20];
#define GN_T0() const uint64_t gn_t0_ = __builtin_readcyclecounter(); uint32_t gn_c_[6] = {0, 0, 0, 0, 0, 0}
#define GN_T(k) do { if (gi < (1 << 20)) { g_gntime[2 * gi + (k)] = (uint32_t)(__builtin_readcyclecounter() - gn_t0_); \
                       if ((k) == 1) for (int q_ = 0; q_ < 6; ++q_) g_gncnt[6 * gi + q_] = gn_c_[q_]; } } while (0)
#define GN_C(k, n) (gn_c_[k] += (n))
#define GN_CLK() __builtin_readcyclecounter()
#else
#define GN_T0() do {} while (0)
#define GN_T(k) do {} while (0)
#define GN_C(k, n) do {} while (0)
#define GN_CLK() 0ull
#endif
template <int K>
__global__ void __launch_bounds__(kGnBT) k_gen_neighbours_lds(const PassConst* __restrict__ pcp, DevBufs B,
                                                              const int* __restrict__ list, const int* __restrict__ nlist_p,
                                                              const float* __restrict__ gtab, int* __restrict__ ovf,
                                                              int* __restrict__ novf) {   // DPE.cu:2103-2463
  __shared__ uint32_t s_pt[K][kGnBT];           // support point (x | y << 16)
  const PassConst& pc = *pcp;
  const int t = threadIdx.x;
  const int gi = xcd_remap(blockIdx.x, gridDim.x, B.xcd_rows * 64) * kGnBT + t;
  if (gi >= *nlist_p) return;
  const int W = pc.W;
  const int center = list[gi];
  const int x = center % W, y = center / W;
  const float depth_diff = pc.P.depth_max - pc.P.depth_min;
  const DpeCamera& camera = pc.cams[0];
  Rng rs; rng_init(rs, (uint32_t)center, pc.seed32, STREAM_GEN_NEIGHBOURS, pc.salt);
  PHASE_BEGIN();
  GN_T0();
  int valid_count = 0;
  bool overflow = false;
  auto push = [&](short2 np) {
    if (valid_count < K) s_pt[valid_count][t] = (uint32_t)(uint16_t)np.x | ((uint32_t)(uint16_t)np.y << 16);
    else overflow = true;
    valid_count++;
  };
  auto pt_at = [&](int i) -> short2 {
    const uint32_t v = s_pt[i][t];
    return make_short2((short)(v & 0xFFFFu), (short)(v >> 16));
  };
  const float ransac_threshold = pc.P.ransac_threshold * depth_diff;
  auto crosses = [&](int ax, int ay, int bx, int by) -> bool { return bresenham(pc, B, ax, ay, bx, by); };
  // complex_new goes to complex_[center] once the pixel is done, never when it is deferred: the
  // rerun draws again from the value this kernel read
  const GnLimit lim = gn_limit_draw(pc, B, center, rs);
  const bool edge_limit = lim.edge_limit;
  const float complex_new = lim.complex_new;
  // The probe's walk pair runs from the pixel: BresenhamLine(A, B) is "an edge on the walk B -> A or
  // on the walk A -> B", whichever is walked first; with the pixel as B the first walk starts at the
  // pixel, where the edge that blocks a direction usually is, and stops there (round 4).
  auto probe_blocked = [&](short2 np) -> bool {
    GN_C(1, 1);
    const uint64_t gn_b0_ = GN_CLK(); (void)gn_b0_;
    const bool hit = crosses(np.x, np.y, x, y);
    GN_C(4, (uint32_t)(GN_CLK() - gn_b0_));
    return hit;
  };
  gn_collect(pc, B, rs, x, y, center, edge_limit, push, probe_blocked,
             [&](int k) { if (k == kGnNoteStep) GN_C(0, 1); else PHASE(0); });
  PHASE(1);
  GN_T(0);
  auto defer = [&]() { ovf[atomicAdd(novf, 1)] = center; PHASE_END_ALL(2); GN_T(1); };
  auto finish_fail = [&]() {
    GN_T(1);
    if (complex_new >= 0.0f) B.complex_[center] = complex_new;
    short2* nb = B.nb + (size_t)center * 9;
    nb[0] = make_short2((short)x, (short)y);
    for (int i = 1; i < 9; ++i) nb[i] = make_short2(-1, -1);
    B.weak_rel[center] = 0;
    PHASE_END_ALL(2);
  };
  if (overflow) { defer(); return; }
  if (valid_count <= 3) { finish_fail(); return; }
  // depths of the support points (the reference's spv3[].z); the 3-D points and normals of the
  // drawn triples are recomputed from (pixel, depth) / planes0[] with the reference's expressions
  auto depth_at = [&](int i) -> float { const uint32_t v = s_pt[i][t]; return B.planes0[(v & 0xFFFFu) + (v >> 16) * W].w; };
  auto point3 = [&](short2 p, int i) -> float3 {
    float Y[3];
    get3d(camera, p.x, p.y, depth_at(i), Y);
    return make_float3(Y[0], Y[1], Y[2]);
  };
  auto normal3 = [&](short2 p) -> float4 { return transform_normal_ref(camera, B.planes0[p.x + p.y * W]); };
  float X[3];
  get3d(camera, x, y, B.planes0[center].w, X);
  const float cpz = X[2];
  auto resid_of = [&](const float4& pl, int si) -> float {
    const uint32_t v = s_pt[si][t];
    return __builtin_fabsf(gn_plane_depth(pl, gtab[v & 0xFFFFu], gtab[W + (v >> 16)]) - depth_at(si));
  };
  PHASE(2);
  float4 best_plane = make_float4(0, 0, 0, 0);
  bool has_valid_plane = false, nan_sort = false;
  {
    int iteration = 50, max_iter = pc.P.high_res_img ? 200 : 125, max_count = 3;
    float min_cost = 3.40282347e+38f;
    float temp_thr = ransac_threshold;
    bool has_consist_normal_plane = false;
    bool must_in_triangle = (pc.P.use_label && B.label[center] > 0 && edge_limit) ? false : true;
    while (iteration > 0 && max_iter > 0) {
      max_iter--;
      GN_C(2, 1);
      int a, b, c;
      if (!gn_draw_triple(rs, valid_count, a, b, c)) continue;
      const short2 pa = pt_at(a), pb = pt_at(b), pcc = pt_at(c);
      if (must_in_triangle && !point_in_triangle(pa, pb, pcc, x, y)) continue;
      if (edge_limit) {
        bool eab, ebc, eca;
        const uint64_t gn_b1_ = GN_CLK(); (void)gn_b1_;
        eab = crosses(pa.x, pa.y, pb.x, pb.y);
        ebc = crosses(pb.x, pb.y, pcc.x, pcc.y);
        eca = crosses(pcc.x, pcc.y, pa.x, pa.y);
        GN_C(3, 3);
        GN_C(5, (uint32_t)(GN_CLK() - gn_b1_));
        if (eab || ebc || eca) continue;
      }
      bool normal_consistency = false;
      if (pc.P.geom_consistency && edge_limit) {
        normal_consistency = gn_normals_agree(normal3(pa), normal3(pb), normal3(pcc));
        if (has_consist_normal_plane && !normal_consistency) continue;
      }
      iteration--;
      bool ok;
      const float4 cv = gn_plane3(point3(pa, a), point3(pb, b), point3(pcc, c), ok);
      if (!ok) continue;
      int temp_count = 0;
      for (int si = 0; si < valid_count; ++si)
        if (resid_of(cv, si) < temp_thr) temp_count++;
      if (temp_count < 6) continue;
      if (temp_count > max_count) {
        if (!must_in_triangle && point_in_triangle(pa, pb, pcc, x, y)) must_in_triangle = true;
        if (!has_consist_normal_plane && normal_consistency) has_consist_normal_plane = true;
        const float cd = gn_centre_cost(camera, cv, x, y, cpz);
        best_plane = cv; max_count = temp_count; min_cost = cd; has_valid_plane = true;
        if ((double)temp_thr > (pc.P.high_res_img ? 0.05 : 0.005)) {
          // sort_small(residuals, valid_count) then residuals[DPE_NEIGHBOUR_NUM] (DPE.cu:5-14,
          // 2367-2376): the 10th smallest residual (0 when there are at most 9: the untouched entry);
          // the count that follows is the number of residuals below the new threshold, all of them
          // among those 10 smallest
          float top[DPE_NEIGHBOUR_NUM + 1];
#pragma unroll
          for (int k = 0; k <= DPE_NEIGHBOUR_NUM; ++k) top[k] = __builtin_inff();
          bool has_nan = false;
          for (int si = 0; si < valid_count; ++si) {
            float r = resid_of(cv, si);
            has_nan |= r != r;
#pragma unroll
            for (int k = 0; k <= DPE_NEIGHBOUR_NUM; ++k) {   // sorted insertion, static indices
              const float lo = __builtin_fminf(top[k], r), hi = __builtin_fmaxf(top[k], r);
              top[k] = lo; r = hi;
            }
          }
          if (has_nan) { nan_sort = true; break; }
          const float kth = valid_count > DPE_NEIGHBOUR_NUM ? top[DPE_NEIGHBOUR_NUM] : 0.0f;
          if (temp_thr < kth) continue;
          temp_thr = (float)((double)kth - 1e-6);
          temp_count = 0;
#pragma unroll
          for (int k = 0; k <= DPE_NEIGHBOUR_NUM; ++k)
            if (k < valid_count && top[k] < temp_thr) temp_count++;
          max_count = temp_count;
        }
      } else if (temp_count == max_count) {
        if (!must_in_triangle && point_in_triangle(pa, pb, pcc, x, y)) must_in_triangle = true;
        const float cd = gn_centre_cost(camera, cv, x, y, cpz);
        if (cd < min_cost) { best_plane = cv; max_count = temp_count; min_cost = cd; }
      }
    }
  }
  PHASE(3);
  if (nan_sort) { defer(); return; }
  if (!has_valid_plane) { finish_fail(); return; }
  // weights (DPE.cu:2437-2449) in place of the depths, then sort_small_weighted (:16-29) and the
  // first 8 points: the insertion sort is stable, so with no NaN weight the k-th output is the k-th
  // smallest (weight, index) -- outliers carry FLT_MAX and the point (-1, -1)
  bool wnan = false;
  for (int i = 0; i < valid_count; ++i) { const float dist = resid_of(best_plane, i); wnan |= dist != dist; }
  auto weight_at = [&](int i) -> float {
    const float dist = resid_of(best_plane, i);
    return dist >= ransac_threshold ? 3.40282347e+38f : dist;
  };
  if (wnan) { defer(); return; }
  short2 out[DPE_NEIGHBOUR_NUM - 1];
  uint64_t taken = 0;
#pragma unroll
  for (int k = 0; k < DPE_NEIGHBOUR_NUM - 1; ++k) {
    int bi = -1; float bw = 0.0f;
    for (int i = 0; i < valid_count; ++i) {
      if ((taken >> i) & 1ull) continue;
      const float w = weight_at(i);
      if (bi < 0 || w < bw) { bi = i; bw = w; }
    }
    if (bi >= 0) { taken |= 1ull << bi; out[k] = bw >= ransac_threshold ? make_short2(-1, -1) : pt_at(bi); }
    else out[k] = make_short2(-1, -1);
  }
  if (complex_new >= 0.0f) B.complex_[center] = complex_new;
  short2* nb = B.nb + (size_t)center * 9;
  nb[0] = make_short2((short)x, (short)y);
#pragma unroll
  for (int k = 0; k < DPE_NEIGHBOUR_NUM - 1; ++k) nb[k + 1] = out[k];
  B.weak_rel[center] = 1;
  PHASE(4);
  PHASE_END_ALL(2);
  GN_T(1);
}

// ------------------------------------------------------------------------------ NeigbourUpdate
__global__ void k_neighbour_update(const PassConst* __restrict__ pcp, DevBufs B) {   // DPE.cu:2465-2481
  const PassConst& pc = *pcp;
  PIX2D_FULL();
  if (B.weak[center] != DPE_WEAK) return;
  if (B.weak_rel[center] != 1) B.weak[center] = DPE_UNKNOWN;
}

// ------------------------------------------------------------------------------ RANSACToGetFitPlane
constexpr int kRansacThreads = 128;   // 1-D workgroups: 16 KB of LDS each
// One thread per entry of a weak list (the sweep's list of one colour), instead of the reference's
// full-grid launch with ~80 % of the threads returning at once.  Only the colour's own weak update
// reads a fit plane or radius, so the rows past the red/black grid (half_rows) need none.
__global__ void __launch_bounds__(kRansacThreads) k_ransac_fit(const PassConst* __restrict__ pcp, DevBufs B, int iter,
                                                               const int* __restrict__ list, const int* __restrict__ nlist_p) {   // DPE.cu:2891-3124
  const PassConst& pc = *pcp;
  const int gi = xcd_remap(blockIdx.x, gridDim.x, B.xcd_rows * 16) * kRansacThreads + (int)threadIdx.x;
  if (gi >= *nlist_p) return;
  const int center = list[gi];
  const int x = center % pc.W, y = center / pc.W;
  const int W = pc.W;
  if (B.weak[center] != DPE_WEAK) return;
  Rng rs; rng_init(rs, (uint32_t)center, pc.seed32, STREAM_ITER_BASE + 4 * iter + 1, pc.salt);
  const DpeCamera& camera = pc.cams[0];
  const bool edge_limit = gn_limit_draw(pc, B, center, rs).edge_limit;   // the fit writes no complex_
  // support points in LDS (thread index fastest): the random draws index them, which a register
  // array cannot do without scratch memory.  Their normals are re-read from the planes when a try
  // needs them (nothing writes a plane during the fits): 128 B of LDS per thread instead of 224, so
  // 5 waves per SIMD instead of 3 and both colours' fits resident at once
  __shared__ short2 s_sp[8][kRansacThreads];
  __shared__ float3 s_sp3[8][kRansacThreads];
  const int tid = threadIdx.x;
  struct Col2 { short2* p; DEV short2& operator[](int i) const { return p[i * kRansacThreads]; } } sp{&s_sp[0][tid]};
  struct Col3 { float3* p; DEV float3& operator[](int i) const { return p[i * kRansacThreads]; } } sp3{&s_sp3[0][tid]};
  auto spn = [&](int i) -> float3 {
    const float4 pl = B.planes[sp[i].x + sp[i].y * W];
    return make_float3(pl.x, pl.y, pl.z);
  };
  int sc = 0;
  float X[3];
  const short2* nb = B.nb + (size_t)center * 9;
  for (int i = 1; i < DPE_NEIGHBOUR_NUM; ++i) {
    const short2 tp = nb[i];
    if (tp.x == -1 || tp.y == -1) continue;
    sp[sc] = tp;
    const float4 pl = B.planes[tp.x + tp.y * W];
    const float depth = depth_from_plane(camera, pl, tp.x, tp.y);
    get3d(camera, tp.x, tp.y, depth, X);
    sp3[sc] = make_float3(X[0], X[1], X[2]);
    sc++;
  }
  if (sc < 3) { B.fit_plane[center] = B.planes[center]; return; }
  int iteration = 50;
  int ua = -1, ub = -1, uc = -1;
  float min_cost = 3.40282347e+38f;
  float4 best = make_float4(0, 0, 0, 0);
  bool has_best = false, has_strong_plane = false;
  bool must_in_triangle = (pc.P.use_label && B.label[center] > 0 && edge_limit) ? false : true;
  // edge_test[8][8] (DPE.cu:2960) as two 64-bit matrices, bit a * 8 + b
  uint64_t tested = 0, crosses = 0;
  auto edge_pair = [&](int a, int b) -> bool {
    if (!((tested >> (a * 8 + b)) & 1ull)) {
      const bool c = bresenham(pc, B, sp[a].x, sp[a].y, sp[b].x, sp[b].y);
      tested |= (1ull << (a * 8 + b)) | (1ull << (b * 8 + a));
      if (c) crosses |= (1ull << (a * 8 + b)) | (1ull << (b * 8 + a));
    }
    return (crosses >> (a * 8 + b)) & 1ull;
  };
  while (iteration--) {
    int a, b, c;
    if (!gn_draw_triple(rs, sc, a, b, c)) continue;
    bool is_strong_plane = false;
    if (pc.P.geom_consistency && edge_limit) {
      is_strong_plane = gn_normals_agree(spn(a), spn(b), spn(c));
      if (has_strong_plane && !is_strong_plane) continue;
    }
    if (must_in_triangle && !point_in_triangle(sp[a], sp[b], sp[c], x, y)) continue;
    if (edge_limit) {
      const bool eab = edge_pair(a, b);
      const bool ebc = edge_pair(b, c);
      const bool eca = edge_pair(c, a);
      if (eab || ebc || eca) continue;
    }
    bool ok;
    const float4 cv = gn_plane3(sp3[a], sp3[b], sp3[c], ok);
    if (!ok) continue;
    if (!has_strong_plane && is_strong_plane) has_strong_plane = true;
    float tcost = 0.0f;
    for (int si = 0; si < sc; ++si) {
      if (si == a || si == b || si == c) continue;
      const float fx = ((float)sp[si].x - camera.K[2]) / camera.K[0];
      const float fy = ((float)sp[si].y - camera.K[5]) / camera.K[4];
      tcost += __builtin_fabsf(gn_plane_depth(cv, fx, fy) - sp3[si].z);
    }
    if (tcost < min_cost) {
      if (!must_in_triangle && point_in_triangle(sp[a], sp[b], sp[c], x, y)) must_in_triangle = true;
      min_cost = tcost; best = cv; has_best = true; ua = a; ub = b; uc = c;
    }
  }
  if (has_best) {
    const float depth = depth_from_plane(camera, B.planes[center], x, y);
    const float4 vd = view_direction(camera, x, y, depth);
    if (best.x * vd.x + best.y * vd.y + best.z * vd.z > 0) { best.x = -best.x; best.y = -best.y; best.z = -best.z; best.w = -best.w; }
    B.fit_plane[center] = best;
    if (pc.P.use_radius) {
      if (must_in_triangle) {
        const short2 A = sp[ua], Bq = sp[ub], C = sp[uc];
        const float a = __builtin_sqrtf((float)((A.x - Bq.x) * (A.x - Bq.x) + (A.y - Bq.y) * (A.y - Bq.y)));
        const float b = __builtin_sqrtf((float)((Bq.x - C.x) * (Bq.x - C.x) + (Bq.y - C.y) * (Bq.y - C.y)));
        const float c = __builtin_sqrtf((float)((C.x - A.x) * (C.x - A.x) + (C.y - A.y) * (C.y - A.y)));
        const float p = (float)((double)(a + b + c) / 2.0);
        const float Sarea = __builtin_sqrtf(p * (p - a) * (p - b) * (p - c));
        int radius = d2i(__builtin_floor((double)__builtin_sqrtf(Sarea) / 2.0));
        const float Ad = __builtin_sqrtf((float)((A.x - x) * (A.x - x) + (A.y - y) * (A.y - y)));
        const float Bd = __builtin_sqrtf((float)((Bq.x - x) * (Bq.x - x) + (Bq.y - y) * (Bq.y - y)));
        const float Cd = __builtin_sqrtf((float)((C.x - x) * (C.x - x) + (C.y - y) * (C.y - y)));
        const float min_dis = MINo(MINo(Ad, Bd), Cd);
        if (2.5 * (double)min_dis < (double)radius) radius = f2i(min_dis);
        if (edge_limit) {
          if (pc.P.use_edge) {
            float med = 3.40282347e+38f;
            const short2* en = B.edge_neigh + (size_t)center * 8;
            for (int d = 0; d < 8; ++d) {
              const short2 ep = en[d];
              if (ep.x == -1 || ep.y == -1) continue;
              const float dist = __builtin_sqrtf((float)((ep.x - x) * (ep.x - x) + (ep.y - y) * (ep.y - y)));
              med = MINo(med, dist);
            }
            if (med < (float)radius) radius = f2i(med);
          }
          if (pc.P.use_label && B.label[center] > 0) {
            float mbd = 3.40282347e+38f;
            const short2* lb = B.lab_bound + (size_t)center * 8;
            for (int d = 0; d < 8; ++d) {
              const short2 bp = lb[d];
              if (bp.x == -1 || bp.y == -1) continue;
              const double dxx = (double)(x - bp.x), dyy = (double)(y - bp.y);
              const float dist = (float)__builtin_sqrt(dxx * dxx + dyy * dyy);
              mbd = MINo(mbd, dist);
            }
            if (mbd < (float)radius) radius = f2i(mbd);
          }
        }
        while ((radius << 1) % 5 != 0) radius--;
        if (!edge_limit) B.radius[center] = radius > pc.P.strong_radius ? 0 : pc.P.strong_radius;
        else B.radius[center] = radius > pc.P.strong_radius ? radius : pc.P.strong_radius;
      } else {
        B.radius[center] = pc.P.strong_radius;
      }
    }
  } else {
    B.fit_plane[center] = make_float4(0, 0, 0, 0);
    if (pc.P.use_radius) B.radius[center] = pc.P.strong_radius;
  }
}

}  // namespace dpe
