// pass_sweep.h — cooperative red/black sweeps (CheckerboardPropagationStrong/Weak, DPE.cu:1214-1862).
//
// The reference runs one thread per pixel with cost_array[8][32] in local memory (DPE.cu:1236, 1690).
// Here a wave owns P pixels and gives each pixel C lanes:
//   strong sweep, edge mode      P = 4,  C = 16 (8 adaptive + 8 fixed 11-step candidates)
//   strong sweep, ACMH mode      P = 8,  C = 8  (near/far candidates)
//   weak sweep                   P = 8,  C = 8  (the 8 deformable neighbours)
// Candidate scans and the candidate x view NCC cost vectors run in parallel lanes; cost vectors
// live in LDS ([pixel][candidate][view], a few KB per wave, so occupancy is register-limited);
// the reference patch (weights, weight*grey) is built once per pixel in LDS.  Every step whose
// floating-point order or RNG order matters (CDF, the 15 view samples, cost sums over views,
// hypothesis acceptance) runs on the pixel's first lane in the reference's order, so results are
// bit-identical to the serial restatement.  Pixels come from per-colour compacted lists.
#pragma once
#include "pass_common.h"
#include "pass_refine.h"
#include "lds_layout.h"
#include "pass_lists.h"
#include "pool_tail.h"

namespace dpe {

// ------------------------------------------------------------------------------ pixel lists
// MODE 0: list[k] (k = colour*2 + weak?1:0) = pixels of that colour and class inside the red/black
//         grid (rows < half_rows), for the sweeps (built after NeigbourUpdate).
// MODE 1: one list of all WEAK pixels (rows < H), for GenNeighbours (built before it).
// MODE 2: colour-0 pixels of the red/black grid whose GenNeighbours failed (weak_rel == 0; the
//         pixels NeigbourUpdate turns UNKNOWN), for the iteration-0 colour-0 strong sweep that runs
//         beside GenNeighbours on the pre-GenNeighbours list (see dpe_pm_execute).
// Row-major order; one wave per row; ballot compaction keeps the order deterministic.
template <int MODE> constexpr int list_count() { return MODE == 0 ? 4 : 1; }
template <int MODE> DEV int list_rows(const PassConst& pc) { return MODE == 1 ? pc.H : pc.half_rows; }
template <int MODE> DEV int list_key(const PassConst& pc, const DevBufs& B, int x, int y) {
  if constexpr (MODE == 2) return (((x + y) & 1) == 0 && B.weak_rel[y * pc.W + x] == 0) ? 0 : -1;
  const bool wk = B.weak[y * pc.W + x] == DPE_WEAK;
  if constexpr (MODE == 1) return wk ? 0 : -1;
  else return (((x + y) & 1) << 1) | (wk ? 1 : 0);
}
template <int MODE>
__global__ void k_list_count(const PassConst* __restrict__ pcp, DevBufs B, int* __restrict__ row_counts) {
  constexpr int NL = list_count<MODE>();
  const PassConst& pc = *pcp;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int y = blockIdx.x * 4 + wave, rows = list_rows<MODE>(pc);
  if (y >= rows) return;
  int cnt[NL];
  for (int j = 0; j < NL; ++j) cnt[j] = 0;
  for (int x0 = 0; x0 < pc.W; x0 += 64) {
    const int x = x0 + lane;
    const int k = x < pc.W ? list_key<MODE>(pc, B, x, y) : -1;
#pragma unroll
    for (int j = 0; j < NL; ++j) cnt[j] += __popcll(__ballot(k == j));
  }
  if (lane == 0)
    for (int j = 0; j < NL; ++j) row_counts[j * rows + y] = cnt[j];
}
// exclusive scan of the row counts of each list: one wave per list, 64 rows per step
template <int MODE>
__global__ void k_list_scan(const PassConst* __restrict__ pcp, int* __restrict__ row_counts, int* __restrict__ totals) {
  const PassConst& pc = *pcp;
  const int j = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int rows = list_rows<MODE>(pc);
  if (j >= list_count<MODE>()) return;
  int acc = 0;
  for (int y0 = 0; y0 < rows; y0 += 64) {
    const int y = y0 + lane;
    const int c = y < rows ? row_counts[j * rows + y] : 0;
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    if (y < rows) row_counts[j * rows + y] = acc + incl - c;
    acc += __shfl(incl, 63);
  }
  if (lane == 0) totals[j] = acc;
}
template <int MODE>
__global__ void k_list_fill(const PassConst* __restrict__ pcp, DevBufs B, const int* __restrict__ row_offsets,
                            int* __restrict__ lists, long list_stride) {
  constexpr int NL = list_count<MODE>();
  const PassConst& pc = *pcp;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int y = blockIdx.x * 4 + wave, rows = list_rows<MODE>(pc);
  if (y >= rows) return;
  int off[NL];
  for (int j = 0; j < NL; ++j) off[j] = row_offsets[j * rows + y];
  const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  for (int x0 = 0; x0 < pc.W; x0 += 64) {
    const int x = x0 + lane;
    const int k = x < pc.W ? list_key<MODE>(pc, B, x, y) : -1;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const unsigned long long m = __ballot(k == j);
      if (k == j) lists[j * list_stride + off[j] + __popcll(m & below)] = y * pc.W + x;
      off[j] += __popcll(m);
    }
  }
}

// ------------------------------------------------------------------------------ weak list by patch side
// The weak sweep's NCC-New cost runs the pixel's centre patch at side n_c (6 at radius >= 5, 1 at the
// radius RANSACToGetFitPlane sets to 0; DPE.cu:1120-1212, 557-690), and a wave runs the sides of its
// pixels one after the other.  After the fits, each colour's weak list is stably partitioned into
// side >= 4 then side < 4 pixels (chunks of kPartChunk entries: count, scan, fill), so almost every
// wave holds one side.  Pixels of a half-sweep are independent, so the order changes no result.
// (kPartChunk: pass_lists.h, which sizes the chunk counts by it)
DEV int weak_side(const PassConst& pc, const DevBufs& B, int center) {
  const int rad = B.radius[center], inc = MAXo(2, d2i(2.0 * rad / 5.0));
  return rad >= 0 ? (2 * rad) / inc + 1 : 0;
}
DEV int part_key(const PassConst& pc, const DevBufs& B, int center) { return weak_side(pc, B, center) >= 4 ? 1 : 0; }
DEV int block_sum256(int v, int* s4) {   // sum over a 256-thread block (all threads call it)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
  __syncthreads();
  const int t = s4[0] + s4[1] + s4[2] + s4[3];
  __syncthreads();
  return t;
}
static __global__ void __launch_bounds__(256) k_part_count(const PassConst* __restrict__ pcp, DevBufs B, const int* __restrict__ list,
                                                    const int* __restrict__ nlist_p, int* __restrict__ chunk_cnt) {
  const PassConst& pc = *pcp;
  const int n = *nlist_p, base = blockIdx.x * kPartChunk;
  if (base >= n) return;   // block-uniform
  __shared__ int s4[4];
  int cnt = 0;
  for (int i = base + (int)threadIdx.x; i < min(n, base + kPartChunk); i += 256) cnt += part_key(pc, B, list[i]);
  cnt = block_sum256(cnt, s4);
  if (threadIdx.x == 0) chunk_cnt[blockIdx.x] = cnt;
}
// exclusive scan of the chunk counts (one 256-thread block); total side->=4 count into *tot
static __global__ void __launch_bounds__(256) k_part_scan(const int* __restrict__ nlist_p, int* __restrict__ chunk_cnt,
                                                   int* __restrict__ tot) {
  __shared__ int s4[4];
  const int nch = (*nlist_p + kPartChunk - 1) / kPartChunk;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int acc = 0;
  for (int k0 = 0; k0 < nch; k0 += 256) {
    const int k = k0 + (int)threadIdx.x;
    const int c = k < nch ? chunk_cnt[k] : 0;
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    if (lane == 63) s4[wave] = incl;
    __syncthreads();
    int before = acc;
    for (int w = 0; w < wave; ++w) before += s4[w];
    const int all = s4[0] + s4[1] + s4[2] + s4[3];
    __syncthreads();
    if (k < nch) chunk_cnt[k] = before + incl - c;
    acc += all;
  }
  if (threadIdx.x == 0) *tot = acc;
}
static __global__ void __launch_bounds__(256) k_part_fill(const PassConst* __restrict__ pcp, DevBufs B, const int* __restrict__ list,
                                                   const int* __restrict__ nlist_p, const int* __restrict__ chunk_off,
                                                   const int* __restrict__ tot, int* __restrict__ out) {
  const PassConst& pc = *pcp;
  const int n = *nlist_p, base = blockIdx.x * kPartChunk;
  if (base >= n) return;
  __shared__ int s4[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int offA = chunk_off[blockIdx.x], offB = *tot + (base - offA);
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  int runA = 0;   // side->=4 entries of this chunk before the current step
  for (int i0 = base; i0 < min(n, base + kPartChunk); i0 += 256) {
    const int i = i0 + (int)threadIdx.x;
    const int p = i < n ? list[i] : 0;
    const int k = i < n ? part_key(pc, B, p) : 0;
    const unsigned long long m = __ballot(k == 1);
    if (lane == 0) s4[wave] = __popcll(m);
    __syncthreads();
    int a = runA + __popcll(m & below);
    for (int w = 0; w < wave; ++w) a += s4[w];
    const int all = s4[0] + s4[1] + s4[2] + s4[3];
    __syncthreads();
    if (i < n) out[k ? offA + a : offB + (i - base) - a] = p;
    runA += all;
  }
}

// ------------------------------------------------------------------------------ view selection
// sampling probability of view i before the prior (DPE.cu:1568-1589), costs by candidate j.
template <class CostF>
DEV float view_prob_raw(CostF cost, int i, float cost_threshold) {
  float count = 0; int count_false = 0; float tmpw = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const float c = cost(j, i);
    if (c < cost_threshold) { tmpw += d_expf(c * c / (-0.18f)); count++; }
    if (c > 1.2f) count_false++;
  }
  float sp = 0.0f;
  if (count > 2 && count_false < 3) sp = tmpw / count;
  else if (count_false < 3) sp = d_expf(cost_threshold * cost_threshold / (-0.32f));
  return sp;
}

// Serial part of the joint view selection on one lane (DPE.cu:1592-1615): CDF over `sp`, 15 samples.
DEV void view_sample(const float* sp, int nv, Rng& rs, uint8_t* vw, uint32_t& tsv, float& wnorm) {
  for (int i = 0; i < DPE_MAX_IMAGES; ++i) vw[i] = 0;
  float psum = 0.0f;
  for (int i = 0; i < nv; ++i) psum += sp[i];
  const float inv = 1.0f / psum;
  float cdf[DPE_MAX_IMAGES];
  float cum = 0.0f;
  for (int i = 0; i < nv; ++i) { const float q = sp[i] * inv; cum += q; cdf[i] = cum; }
  for (int s = 0; s < 15; ++s) {
    const float rp = rng_uniform(rs) - 1.1920929e-07f;
    for (int id = 0; id < nv; ++id)
      if (cdf[id] > rp) { vw[id] += 1; break; }
  }
  uint32_t t = 0; float wn = 0;
  for (int i = 0; i < nv; ++i) if (vw[i] > 0) { setBit(t, i); wn += vw[i]; }
  tsv = t; wnorm = wn;
}

// The same sampling on the C lanes of one pixel: the CDF is built in the reference's order on lane
// 0 (in place of sp), the 15 draws (stream words 0..14) and their CDF searches run one per lane,
// and the per-view counts are LDS integer atomics (order-free).  cnt: nv ints of scratch.
// Leaves vwl[0..31] and the global copy vwg[0..31]; the caller's lane-0 stream is then positioned
// with rng_seek(rs, 15).  Every lane of the wave calls it (wave_sync inside).
DEV void view_sample_coop(float* sp, int* cnt, int nv, int c, int C, bool active, const Rng& rs, uint8_t* vwl,
                          uint8_t* vwg) {
  if (active) {
    if (c == 0) {
      float psum = 0.0f;
      for (int i = 0; i < nv; ++i) psum += sp[i];
      const float inv = 1.0f / psum;
      float cum = 0.0f;
      for (int i = 0; i < nv; ++i) { const float q = sp[i] * inv; cum += q; sp[i] = cum; }
    }
    for (int v = c; v < nv; v += C) cnt[v] = 0;
  }
  wave_sync();
  if (active) {
    for (int s = c; s < 15; s += C) {
      const float rp = u32_to_uniform(rng_word(rs, (uint32_t)s)) - 1.1920929e-07f;
      for (int id = 0; id < nv; ++id)
        if (sp[id] > rp) { atomicAdd(&cnt[id], 1); break; }
    }
  }
  wave_sync();
  if (active)
    for (int j = c; j < DPE_MAX_IMAGES; j += C) {
      const uint8_t w = j < nv ? (uint8_t)cnt[j] : (uint8_t)0;
      vwl[j] = w;
      vwg[j] = w;
    }
  wave_sync();
}

// ------------------------------------------------------------------------------ candidate scans
// Edge-adaptive (kind 0) and fixed 11-step (kind 1) scans of direction d (DPE.cu:1250-1292, 1297-1322).
DEV int edge_candidate(const PassConst& pc, const DevBufs& B, const float* __restrict__ costs, int x, int y, int center,
                       int iter, int d, int kind, bool on_edge) {
  const int W = pc.W, H = pc.H;
  const int dx = kDir[d][0], dy = kDir[d][1];
  const int s0 = MAXo(1, 5 - 2 * iter);
  const int min_step_len = 2;
  int step_num = 11, step_len = min_step_len;
  if (kind == 0) {
    const float max_edge_dist = MAXo(H, W) / 30.0f;
    const short2 ep = B.edge_neigh[(size_t)center * 8 + d];
    const double ex = (double)(ep.x - x), ey = (double)(ep.y - y);
    float dist = (float)__builtin_sqrt(ex * ex + ey * ey);
    if (d >= 4) dist = (float)((double)dist / 1.4142135623730951);
    if (on_edge) dist = 11 * min_step_len;
    else if (ep.x == -1 || ep.y == -1 || dist > max_edge_dist) {
      dist = max_edge_dist;
      if (d >= 4) dist = (float)((double)dist / 1.4142135623730951);
    }
    step_num = MINo(MAXo(11, f2i(1.0f * dist / min_step_len)), 22);
    step_len = MAXo(f2i(1.0f * dist / step_num), min_step_len);
    if (d < 4 && step_len % 2 == 1) step_len -= 1;
  }
  int fx = 0, fy = 0;
  if (d > 4) { if (d % 2) fx = dx; else fy = dy; }
  int mpos = -1; float mc = 3.40282347e+38f;
  // the loads of 8 steps are issued together, then scanned in step order (same first minimum)
  for (int s = 0; s < step_num; s += 8) {
    float cv[8]; int pv[8]; bool ok[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int step = s + u;
      const int tx = x + s0 * dx + step * step_len * dx + fx, ty = y + s0 * dy + step * step_len * dy + fy;
      ok[u] = step < step_num && tx >= 0 && ty >= 0 && tx < W && ty < H;
      pv[u] = tx + ty * W;
      cv[u] = ok[u] ? costs[pv[u]] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (ok[u] && mc > cv[u]) { mpos = pv[u]; mc = cv[u]; }
  }
  return mc < 3.40282347e+38f ? mpos : -1;
}

// ACMH near/far candidate of slot s (DPE.cu:1346-1544): 0 up_near, 1 up_far, 2 down_near,
// 3 down_far, 4 left_near, 5 left_far, 6 right_near, 7 right_far.  -1 if the slot is absent.
DEV int acmh_candidate(const PassConst& pc, const float* __restrict__ costs, int x, int y, int center, int s) {
  const int W = pc.W, H = pc.H;
  float costMin; int cmp;
  switch (s) {
    case 1: {
      if (!(y > 2)) return -1;
      const int up_far = center - 3 * W; costMin = costs[up_far]; cmp = up_far;
      for (int i = 1; i < 11; ++i) if (y > 2 + 2 * i) { const int pt = up_far - 2 * i * W; if (costs[pt] < costMin) { costMin = costs[pt]; cmp = pt; } }
      return cmp;
    }
    case 3: {
      if (!(y < H - 3)) return -1;
      const int down_far = center + 3 * W; costMin = costs[down_far]; cmp = down_far;
      for (int i = 1; i < 11; ++i) if (y < H - 3 - 2 * i) { const int pt = down_far + 2 * i * W; if (costs[pt] < costMin) { costMin = costs[pt]; cmp = pt; } }
      return cmp;
    }
    case 5: {
      if (!(x > 2)) return -1;
      const int left_far = center - 3; costMin = costs[left_far]; cmp = left_far;
      for (int i = 1; i < 11; ++i) if (x > 2 + 2 * i) { const int pt = left_far - 2 * i; if (costs[pt] < costMin) { costMin = costs[pt]; cmp = pt; } }
      return cmp;
    }
    case 7: {
      if (!(x < W - 3)) return -1;
      const int right_far = center + 3; costMin = costs[right_far]; cmp = right_far;
      for (int i = 1; i < 11; ++i) if (x < W - 3 - 2 * i) { const int pt = right_far + 2 * i; if (costs[pt] < costMin) { costMin = costs[pt]; cmp = pt; } }
      return cmp;
    }
    case 0: {
      if (!(y > 0)) return -1;
      const int up_near = center - W; costMin = costs[up_near]; cmp = up_near;
      for (int i = 0; i < 3; ++i) {
        if (y > 1 + i && x > i) { const int pt = up_near - (1 + i) * W - (1 + i); if (costs[pt] < costMin) { costMin = costs[pt]; cmp = pt; } }
        if (y > 1 + i && x < W - 1 - i) { const int pt = up_near - (1 + i) * W + (1 + i); if (costs[pt] < costMin) { costMin = costs[pt]; cmp = pt; } }
      }
      return cmp;
    }
    case 2: {
      if (!(y < H - 1)) return -1;
      const int down_near = center + W; costMin = costs[down_near]; cmp = down_near;
      for (int i = 0; i < 3; ++i) {
        if (y < H - 2 - i && x > i) { const int pt = down_near + (1 + i) * W - (1 + i); if (costs[pt] < costMin) { costMin = costs[pt]; cmp = pt; } }
        if (y < H - 2 - i && x < W - 1 - i) { const int pt = down_near + (1 + i) * W + (1 + i); if (costs[pt] < costMin) { costMin = costs[pt]; cmp = pt; } }
      }
      return cmp;
    }
    case 4: {
      if (!(x > 0)) return -1;
      const int left_near = center - 1; costMin = costs[left_near]; cmp = left_near;
      for (int i = 0; i < 3; ++i) {
        if (x > 1 + i && y > i) { const int pt = left_near - (1 + i) - (1 + i) * W; if (costs[pt] < costMin) { costMin = costs[pt]; cmp = pt; } }
        if (x > 1 + i && y < H - 1 - i) { const int pt = left_near - (1 + i) + (1 + i) * W; if (costs[pt] < costMin) { costMin = costs[pt]; cmp = pt; } }
      }
      return cmp;
    }
    default: {   // 6
      if (!(x < W - 1)) return -1;
      const int right_near = center + 1; costMin = costs[right_near]; cmp = right_near;
      for (int i = 0; i < 3; ++i) {
        if (x < W - 2 - i && y > i) { const int pt = right_near + (1 + i) - (1 + i) * W; if (costs[pt] < costMin) { costMin = costs[pt]; cmp = pt; } }
        if (x < W - 2 - i && y < H - 1 - i) { const int pt = right_near + (1 + i) + (1 + i) * W; if (costs[pt] < costMin) { costMin = costs[pt]; cmp = pt; } }
      }
      return cmp;
    }
  }
}

// ------------------------------------------------------------------------------ strong sweep
constexpr int kTailJobs = kTailLdsJobs;   // the carve's tail region holds 18 floats for each (pool_tail.h)
// the strong sweep's LDS carve per wave (lds_layout.h: P pixels, C candidate lanes, nv source views)
template <int P, int C> using StrongCarveT = lds::StrongCarve<P, C, kTailJobs>;
__host__ __device__ inline int strong_lds_per_wave(int P, int C, int nv) {
  return P == 4 && C == 16 ? StrongCarveT<4, 16>::total(nv) : StrongCarveT<8, 8>::total(nv);
}
// A wave's block of that carve: typed pointers to pixel q's part of each region (q = 0..P-1; a lane's
// own pixel and, in the job pools, any other).  Holds the block's base and nv, nothing else: every
// address is computed from the layout's offsets where it is used.
template <int P, int C>
struct StrongWave {
  using SC = StrongCarveT<P, C>;
  float* wl;
  int nv;
  DEV float4* hyp(int q) const { return (float4*)(wl + SC::hyp()) + q * 5; }                 // [5] refinement hypotheses
  DEV float* patch(int q) const { return wl + SC::patch() + q * SC::kPatch; }                // [108] reference patch
  DEV float* cost(int q) const { return wl + SC::cost(nv) + q * (C + 1) * nv; }              // [C + 1][nv]; slot C = the current plane
  DEV float* sp(int q) const { return wl + SC::sp(nv) + q * nv; }                            // [nv] view probabilities
  DEV float* ref(int q) const { return wl + SC::ref(nv) + q * 5 * nv; }                      // [5][nv] refinement NCCs (+ sampling counts)
  DEV int* sample_counts(int q) const { return (int*)ref(q); }                                // [nv] view_sample_coop's counts (over ref)
  DEV float* fc(int q) const { return wl + SC::fc(nv) + q * 8; }                             // [8] final costs
  DEV float* sums(int q) const { return wl + SC::sums(nv) + q * 4; }                         // patch sums s_ref, s_rr, s_w; wnorm
  DEV uint8_t* vw(int q) const { return (uint8_t*)(wl + SC::vw(nv)) + q * 32; }              // [32] view weights
  DEV int* ib(int q) const { return (int*)(wl + SC::ib(nv)) + q * SC::ib_ints(nv); }
  DEV int* pos(int q) const { return ib(q) + SC::IB_POS; }                                   // [C] candidate positions (-1 = none)
  DEV int* fin(int q) const { return ib(q) + SC::IB_FIN; }                                   // [8] final slot of direction d (-1 = zero vector)
  DEV int* misc(int q) const { return ib(q) + SC::IB_MISC; }                                 // [8] MI_* slots
  DEV int* sel_list(int q) const { return ib(q) + SC::IB_SEL; }                              // [nv] selected views
  DEV int* slots(int q) const { return ib(q) + SC::ib_slots(nv); }                           // [C + 1] cost-vector jobs: candidate slots, then C
  DEV float4* cpl(int q) const { return (float4*)(wl + SC::cpl(nv)) + q * (C + 1); }         // [C + 1] candidate planes, slot C = current
  DEV int* alias(int q) const { return (int*)(wl + SC::alias(nv)) + q * (C + 1); }           // [C + 1]
  DEV float* rnd(int q) const { return wl + SC::rnd(nv) + q * 12; }                          // [12] refinement draws
  DEV float* tail() const { return wl + SC::tail(nv); }                                      // the split last rounds' row sums
  DEV int& nsel(int q) const { return misc(q)[SC::MI_NSEL]; }                                // selected views
  DEV int& jobs(int q) const { return misc(q)[SC::MI_JOBS]; }                                // cost-vector job slots (candidates + current)
  DEV float& wnorm(int q) const { return sums(q)[3]; }
  DEV float depth(int q, int h) const { return __int_as_float(misc(q)[SC::MI_DEPTH + h]); }  // depth of hypothesis h
  DEV void set_depth(int q, int h, float d) const { misc(q)[SC::MI_DEPTH + h] = __float_as_int(d); }
};

// Job pools of a wave: the NCCs of all its pixels are dealt round-robin over the 64 lanes, so a
// lane's work does not depend on how many candidates / selected views its own pixel has.
// (pixel p, item i) <- flat job j, given per-pixel job counts cnt[p].
template <int P>
DEV bool job_decode(const int* cnt, int j, int& p, int& r) {
  r = j;
#pragma unroll
  for (int q = 0; q < P; ++q) {
    if (r < cnt[q]) { p = q; return true; }
    r -= cnt[q];
  }
  return false;
}

// One job of a pool's last round: the Old NCC of plane `pl` in view v at pixel (qx, qy), reference
// patch `pw` with ncc_pre sums `sm`; its cost goes to *out.
struct TailJob {
  const float* pw; const float* sm; float* out;
  int qx, qy, v;
  float4 pl;
};
#if DPE_POOL_STATS   // tools/pool_stats.py: last rounds of pool k by lanes per job: [k][0] 6, [1] 3, [2] 2, [3] unsplit
static __device__ unsigned long long g_tail[2][4];
#define TAIL_STAT(k, npc) do { if ((threadIdx.x & 63) == 0) atomicAdd(&g_tail[k][(npc) == 6 ? 0 : (npc) == 3 ? 1 : (npc) == 2 ? 2 : 3], 1ull); } while (0)
#else
#define TAIL_STAT(k, npc) do {} while (0)
#endif
// A pool's last round of `tail` <= kTailMaxJobs jobs (fast patches), split by patch rows over the
// lanes as pool_tail.h maps them; every lane of the wave calls this, converged.  job(t) describes
// job t of the round.  A lane computes its rows with lds_row (the operations of lds_taps); the row
// triplets are added to zero in row order as lds_taps adds them, so the cost has ncc_old_lds's bits.
// With two lanes per job the first lane's partial (rows 0..2) goes to the second by a lane shuffle
// and the second adds its rows 3..5 to it; otherwise all six triplets meet in LDS (`tb`, the carve's
// tail region) and the job's last lane adds them.
template <int U8, class JobFn>
DEV void pool_tail_split(int tail, int lane, float* tb, const PassConst& pc, const DevBufs& B, JobFn job) {
  const TailLane tl = tail_lane(tail, lane);
  const bool two = tail_lanes_per_job(tail) == 2;
  TailJob J = {};
  bool outside = true;
  float acc[3] = {0.0f, 0.0f, 0.0f};
  if (tl.job >= 0) {
    J = job(tl.job);
    const Homog H = make_homography(pc, J.v, J.pl);
    bool fr;
    outside = center_outside_patch(pc, J.v, H, J.qx, J.qy, fr);
    if (!outside) {
      for (int a = tl.row0; a < tl.row0 + tl.rows; ++a) {
        float r3[3];
        if (fr) lds_row<U8, true>(J.pw, J.qx, J.qy, pc, B, J.v, H, a, r3);
        else lds_row<U8, false>(J.pw, J.qx, J.qy, pc, B, J.v, H, a, r3);
        if (two && !tl.last) { acc[0] += r3[0]; acc[1] += r3[1]; acc[2] += r3[2]; }
        else { float* t3 = tb + tail_lds_slot(tail, tl.job, a); t3[0] = r3[0]; t3[1] = r3[1]; t3[2] = r3[2]; }
      }
    }
  }
  // the partial of the lane below (the same job's first lane when this is its second)
  const int below = lane > 0 ? lane - 1 : 0;
  const float p0 = __shfl(acc[0], below), p1 = __shfl(acc[1], below), p2 = __shfl(acc[2], below);
  wave_sync();
  if (tl.job >= 0 && tl.last) {
    float cst = 2.0f;
    if (outside) {
      count_work(B, 1, 0);
    } else {
      count_work(B, 1, 36);
      float s_src = two ? p0 : 0.0f, s_ss = two ? p1 : 0.0f, s_rs = two ? p2 : 0.0f;
      for (int a = two ? 3 : 0; a < 6; ++a) {
        const float* r3 = tb + tail_lds_slot(tail, tl.job, a);
        s_src += r3[0]; s_ss += r3[1]; s_rs += r3[2];
      }
      cst = ncc_finalize_pre(J.sm[0], J.sm[1], J.sm[2], s_src, s_ss, s_rs);
    }
    *J.out = cst;
  }
}

// ---- the strong sweep's per-pixel phases.  None holds a barrier: k_strong_coop puts one after each.
// Those that say "converged" use a ballot or a shuffle, so every lane of the wave calls them.

// 31-bit hash of a plane's bits
DEV int plane_hash(const float4& p) {
  uint32_t h = __float_as_uint(p.x) * 0x9E3779B1u;
  h = (h ^ (h >> 15) ^ __float_as_uint(p.y)) * 0x85EBCA77u;
  h = (h ^ (h >> 13) ^ __float_as_uint(p.z)) * 0xC2B2AE3Du;
  h = (h ^ (h >> 16) ^ __float_as_uint(p.w)) * 0x27D4EB2Fu;
  return (int)((h ^ (h >> 15)) & 0x7FFFFFFFu);
}
// phase 1: lane c's candidate position, its plane and the plane's hash; lane 0 adds the current plane
template <bool EDGE, int P, int C>
DEV void strong_candidate(const StrongWave<P, C>& sw, int ps, int c, const PassConst& pc, const DevBufs& B, int x, int y,
                          int center, int iter, bool on_edge) {
  const float4* __restrict__ planes_s = B.planes_snap;
  int pos;
  if constexpr (EDGE) {
    const int d = c & 7, kind = c >> 3;
    pos = (kind == 1 && on_edge) ? -1 : edge_candidate(pc, B, B.costs_snap, x, y, center, iter, d, kind, on_edge);
  } else {
    pos = acmh_candidate(pc, B.costs_snap, x, y, center, c);
  }
  sw.pos(ps)[c] = pos;
  if (pos >= 0) { const float4 pl = planes_s[pos]; sw.cpl(ps)[c] = pl; sw.alias(ps)[c] = plane_hash(pl); }
  else sw.alias(ps)[c] = (int)(0x80000000u | (uint32_t)c);
  if (c == 0) { const float4 pl = planes_s[center]; sw.cpl(ps)[C] = pl; sw.alias(ps)[C] = plane_hash(pl); }
}
// phase 1b: bitwise-identical planes among the candidates and the current plane (a third of the
// candidates in a converged map: propagation copies planes) share one cost vector.  alias[] holds
// the 31-bit hash of each valid slot's plane (absent slots: a unique value with the top bit set); the
// earliest equal-hash slot is confirmed bit by bit.  al[r]: the alias of slot c + r C (-1: absent).
template <int P, int C>
DEV void strong_alias_search(const StrongWave<P, C>& sw, int ps, int c, int (&al)[2]) {
  const int* alias = sw.alias(ps);
  const float4* cpl = sw.cpl(ps);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int sl = c + r * C;
    if (sl > C || (sl < C && sw.pos(ps)[sl] < 0)) continue;
    const float4 me = cpl[sl];
    const uint32_t h = (uint32_t)alias[sl];
    uint32_t m = 0;
#pragma unroll
    for (int t = 0; t < C; ++t) m |= ((uint32_t)alias[t] == h && t < sl) ? (1u << t) : 0u;
    int a = sl;
    while (m) {
      const int t = __builtin_ctz(m);
      if (same_plane_bits(cpl[t], me)) { a = t; break; }
      m &= m - 1;
    }
    al[r] = a;
  }
}
// The cost-vector job slots (k with alias[k] == k, ascending) and, on lane 0, the patch sums.
// SPREAD (converged): lane c owns slot c, and its place in the list is the number of owners below it
// among the pixel's lanes; slot C (the current plane) goes last.  Otherwise lane 0 scans the slots.
template <bool SPREAD, int P, int C>
DEV void strong_slot_list(const StrongWave<P, C>& sw, int ps, int c, int lane, bool active, bool fast) {
  const int* alias = sw.alias(ps);
  int* slots = sw.slots(ps);
  int n = 0;
  if constexpr (SPREAD) {
    const bool own = active && alias[c] == c;
    const uint32_t bits = (uint32_t)(__ballot(own) >> (lane - c)) & ((1u << C) - 1u);
    if (own) slots[__popc(bits & ((1u << c) - 1u))] = c;
    n = __popc(bits);
  }
  if (c == 0) {
    if (active) {
      if constexpr (SPREAD) { if (alias[C] == C) slots[n++] = C; }
      else for (int k = 0; k <= C; ++k) if (alias[k] == k) slots[n++] = k;
      float* sums = sw.sums(ps);
      if (fast) patch_lds_pre(sw.patch(ps), sums[0], sums[1], sums[2]);
    }
    sw.jobs(ps) = n;
  }
}
// duplicates take their original's cost vector
template <int P, int C>
DEV void strong_copy_aliased(const StrongWave<P, C>& sw, int ps, int c) {
  float* cost = sw.cost(ps);
  const int nv = sw.nv;
  for (int sl = c; sl <= C; sl += C) {
    const int a = sw.alias(ps)[sl];
    if (a >= 0 && a != sl)
      for (int v = 0; v < nv; ++v) cost[sl * nv + v] = cost[a * nv + v];
  }
}
// phase 3: the final slot of direction d: in edge mode the arbitration of its two candidates
// (DPE.cu:1323-1342)
template <bool EDGE, int P, int C>
DEV void strong_arbitrate(const StrongWave<P, C>& sw, int ps, int d, int iter, bool on_edge) {
  const int* posl = sw.pos(ps);
  if constexpr (EDGE) {
    const float* cost = sw.cost(ps);
    const int nv = sw.nv;
    const bool hasA = posl[d] >= 0, hasB = !on_edge && posl[8 + d] >= 0;
    int f = hasA ? d : -1;
    if (hasB) {
      const float good_threshold = 0.8f * d_expf((float)(iter * iter) / (-90.0f));
      int g0 = 0, g1 = 0, b0 = 0, b1 = 0;
      for (int j = 0; j < nv; ++j) {
        // slot A as the reference sees it: its vector, or the zero-initialised row
        const float v0 = hasA ? cost[d * nv + j] : ((d == 0 && j == 0) ? 2.0f : 0.0f);
        if (v0 < good_threshold) g0++;
        if (v0 > 1.2f) b0++;
        const float v1 = cost[(8 + d) * nv + j];
        if (v1 < good_threshold) g1++;
        if (v1 > 1.2f) b1++;
      }
      if (!hasA || g1 > g0 || (g1 == g0 && b1 < b0)) f = 8 + d;
    }
    sw.fin(ps)[d] = f;
  } else {
    sw.fin(ps)[d] = posl[d] >= 0 ? d : -1;
  }
}
// cost of (direction j, view i) as the reference's cost_array holds it
template <int P, int C>
DEV float strong_dir_cost(const StrongWave<P, C>& sw, int ps, int j, int i) {
  const int f = sw.fin(ps)[j];
  return f >= 0 ? sw.cost(ps)[f * sw.nv + i] : ((j == 0 && i == 0) ? 2.0f : 0.0f);
}
// phase 4: per-view sampling probabilities with the 4-neighbour priors (DPE.cu:1552-1590)
template <int P, int C>
DEV void strong_view_probs(const StrongWave<P, C>& sw, int ps, int c, const PassConst& pc, const DevBufs& B, int center,
                           int iter) {
  const int W = pc.W, nv = sw.nv;
  const int* fin = sw.fin(ps);
  float* sp = sw.sp(ps);
  const float cost_threshold = (float)(0.8 * (double)d_expf((float)(iter * iter) / (-90.0f)));
  const long Lp = (long)W * pc.H;
  uint32_t nsv[4];
  bool nfl[4];
  const long npos[4] = {(long)center - W, (long)center + W, (long)center - 1, (long)center + 1};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    nfl[i] = fin[2 * i] >= 0;
    nsv[i] = (nfl[i] && npos[i] >= 0 && npos[i] < Lp) ? B.sel_snap[npos[i]] : 0u;
  }
  for (int v = c; v < nv; v += C) {
    float prior = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) if (nfl[i]) prior += isSet(nsv[i], v) == 1 ? 0.9f : 0.1f;
    sp[v] = view_prob_raw([&](int j, int i) { return strong_dir_cost(sw, ps, j, i); }, v, cost_threshold) * prior;
  }
}
// The selected views (vw > 0) as a mask, a list and the weight norm, after the sampling.  SPREAD
// (converged): C views per ballot, view v's place in the list is the number of selected views below
// it, and wnorm adds integers below 2^24: exact, so the order is free.  Otherwise lane 0 scans them.
// tsv and wnorm are lane 0's; the lane's stream is left after the 15 sampling words.
template <bool SPREAD, int P, int C>
DEV void strong_selected_views(const StrongWave<P, C>& sw, int ps, int c, int lane, bool active, Rng& rs, uint32_t& tsv,
                               float& wnorm) {
  const int nv = sw.nv;
  const uint8_t* vwl = sw.vw(ps);
  int* sel_list = sw.sel_list(ps);
  if constexpr (SPREAD) {
    for (int v0 = 0; v0 < nv; v0 += C) {
      const bool on = active && v0 + c < nv && vwl[v0 + c] > 0;
      tsv |= ((uint32_t)(__ballot(on) >> (lane - c)) & ((1u << C) - 1u)) << v0;
    }
    for (int v = c; v < nv; v += C)
      if (isSet(tsv, v)) sel_list[__popc(tsv & ((1u << v) - 1u))] = v;
  }
  if (c == 0) {
    int ns = 0;
    if (active) {
      rng_seek(rs, 15);
      if constexpr (SPREAD) {
        int wi = 0;
        for (int i = 0; i < nv; ++i) wi += vwl[i];
        wnorm = (float)wi;
      } else {
        for (int i = 0; i < nv; ++i) if (vwl[i] > 0) { setBit(tsv, i); wnorm += vwl[i]; sel_list[ns++] = i; }
      }
      sw.wnorm(ps) = wnorm;
    }
    sw.nsel(ps) = SPREAD ? __popc(tsv) : ns;
  }
}
// phase 5: the final cost of direction d over the sampled views
template <int P, int C>
DEV void strong_final_cost(const StrongWave<P, C>& sw, int ps, int d) {
  const int nv = sw.nv;
  const uint8_t* vwl = sw.vw(ps);
  float wn = 0.0f;
  for (int i = 0; i < nv; ++i) wn += vwl[i];   // == weight_norm (same order: sum of vw > 0)
  float f = 0.0f;
  for (int j = 0; j < nv; ++j) { const int w = vwl[j]; if (w > 0) f += w * strong_dir_cost(sw, ps, d, j); }
  sw.fc(ps)[d] = f / wn;
}
// The five hypotheses on lanes 0..4 of the pixel, one each, from lane 0's accepted plane and depth
// (converged): (normal, depth) = (now, rand), (rand, now), (rand, rand), (perturbed, now),
// (now, perturbed).  Lanes 1..3 share one view_direction call (at depth_now, or at 1 for the
// perturbed normal).
template <int P, int C>
DEV void strong_hypotheses_spread(const StrongWave<P, C>& sw, int ps, int c, int lane, bool active, const PassConst& pc,
                                  int x, int y, const float4& pnow, float depth_now) {
  const DpeCamera& c0 = pc.cams[0];
  const float* rnd = sw.rnd(ps);
  const int l0 = lane - c;
  const float4 pn = make_float4(__shfl(pnow.x, l0), __shfl(pnow.y, l0), __shfl(pnow.z, l0), __shfl(pnow.w, l0));
  const float dn = __shfl(depth_now, l0);
  if (active && c < 5) {
    float4 h = pn;
    if (c >= 1 && c <= 3) {
      const float4 vd = view_direction(c0, x, y, c == 3 ? 1.0f : dn);
      h = c == 3 ? perturbed_normal_vd(vd, pn, rnd + 5) : random_normal_vd(vd, rnd + 1);
    }
    float dep = dn;
    if (c == 0 || c == 2) {
      const float dmin = pc.P.depth_min, dmax = pc.P.depth_max;
      dep = rnd[0] * (dmax - dmin) + dmin;
    } else if (c == 4) {
      const float dminp = (1 - 0.02f) * dn, dmaxp = (1 + 0.02f) * dn;
      dep = rnd[4] * (dmaxp - dminp) + dminp;
    }
    h.w = dist2origin(c0, x, y, dep, h);
    sw.hyp(ps)[c] = h;
  }
}

// waves per workgroup: 2 (4 before round 5's end; 2 fits the first half-sweep beside GenNeighbours
// better: wall -0.6 ms together with DepthToWeak at 1, profiles/r05ao_ab_wgsize2.log)
constexpr int kBwStrong = 2;
template <int U8, bool EDGE>
__global__ void __launch_bounds__(64 * kBwStrong, kTapWaves) k_strong_coop(const PassConst* __restrict__ pcp, DevBufs B, int iter,
                                                     const int* __restrict__ list, const int* __restrict__ nlist_p) {
  extern __shared__ float4 lds4[];
  float* lds = (float*)lds4;
  const int nlist = *nlist_p;
  constexpr int C = EDGE ? 16 : 8;
  constexpr int P = 64 / C;
  // the sections that used to run on one lane per pixel (slot list, selected-view list, refinement
  // hypotheses) spread over the pixel's lanes.  Not in the f32-texel instantiation, which has no
  // registers to spare: its edge-mode kernel went from 0 to 8 B/lane of scratch with them.
  constexpr bool kSpread = U8 != TEX_F32;
  // likewise the wider pool tails (last rounds of 17..32 jobs split, and the refinement pool's split
  // at all): 8 B/lane of scratch in the same kernel
  constexpr bool kWideTails = U8 != TEX_F32;
  const PassConst& pc = *pcp;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ps = lane / C, c = lane % C;
  const int W = pc.W, nv = pc.N - 1;
  const DpeCamera& c0 = pc.cams[0];
  const int wbase = (xcd_remap(blockIdx.x, gridDim.x, B.xcd_rows * 16) * kBwStrong + wave) * P;
  if (wbase >= nlist) return;                          // wave-uniform tail
  const int gi = wbase + ps;
  const bool active = gi < nlist;
  const int center = active ? list[gi] : 0;
  const int x = center % W, y = center / W;
  // the wave's LDS carve (lds_layout.h): pixel ps is the lane's own, the pools read any pixel q
  const StrongWave<P, C> sw{lds + (size_t)wave * StrongCarveT<P, C>::total(nv), nv};
  const bool fast = FAST_PATCH(pc);
  const float dmin = pc.P.depth_min, dmax = pc.P.depth_max;
  bool on_edge = false;
  PHASE_BEGIN();
  // ---- phase 1: reference patch + candidate scans
  if (active) {
    if (fast) patch_lds_build<C>(sw.patch(ps), pc, B, x, y, c);
    PHASE(14);
    if constexpr (EDGE) on_edge = B.edge[center] != 0;
    strong_candidate<EDGE>(sw, ps, c, pc, B, x, y, center, iter, on_edge);
  }
  wave_sync();
  PHASE(0);
  // ---- phase 1b: slots with bitwise-identical planes share one cost vector
  int al[2] = {-1, -1};
  if (active) strong_alias_search(sw, ps, c, al);
  wave_sync();
  if (active) {
    sw.alias(ps)[c] = al[0];
    if (c == 0) sw.alias(ps)[C] = al[1];
  }
  wave_sync();
  PHASE(1);
  strong_slot_list<kSpread>(sw, ps, c, lane, active, fast);
  wave_sync();
  PHASE(2);
  // ---- phase 2: cost vectors of every candidate and of the current plane, one flat pool
  {
    // view-major order: the lanes of one round gather from the same source image (cache locality)
    int cnt[P], S = 0;
#pragma unroll
    for (int q = 0; q < P; ++q) { cnt[q] = sw.jobs(q); S += cnt[q]; }
    int q, r;
    const int total = S * nv, tail = total & 63;
    // a last round of at most kTailMaxJobs jobs is split by patch rows (pool_tail_split)
    constexpr int kMaxTail = kWideTails ? kTailMaxJobs : kTailLdsJobs;
    const bool split = fast && tail > 0 && tail <= kMaxTail;
    POOL_STAT(0, total);
    if (tail > 0) TAIL_STAT(0, split ? tail_lanes_per_job(tail) : 1);
    const int jend = split ? total - tail : total;
    // cost-vector job j as the split last round sees it: slot list entry j % S of view j / S + 1
    // (the whole rounds below spell the same job out: through cv_job the ACMH quarter-integer kernel
    // spills 8 B/lane)
    auto cv_job = [&](int j) {
      job_decode<P>(cnt, j % S, q, r);
      const int slot = sw.slots(q)[r], v = j / S + 1;
      const int cq = list[wbase + q];
      return TailJob{sw.patch(q), sw.sums(q), sw.cost(q) + slot * nv + v - 1, cq % W, cq / W, v, sw.cpl(q)[slot]};
    };
    for (int j = lane; j < jend; j += 64) {
      job_decode<P>(cnt, j % S, q, r);
      const int slot = sw.slots(q)[r], v = j / S + 1;
      const int cq = list[wbase + q];
      const float* sm = sw.sums(q);
      sw.cost(q)[slot * nv + v - 1] =
          ncc_old_any<U8>(fast, sw.patch(q), sm[0], sm[1], sm[2], cq % W, cq / W, pc, B, v, sw.cpl(q)[slot]);
    }
    if (split) pool_tail_split<U8>(tail, lane, sw.tail(), pc, B, [&](int t) { return cv_job(jend + t); });
  }
  wave_sync();
  PHASE(3);
  if (active) strong_copy_aliased(sw, ps, c);
  wave_sync();
  PHASE(4);
  // ---- phase 3: arbitration of the two candidates of each direction (edge mode, DPE.cu:1323-1342)
  if (active && c < 8) strong_arbitrate<EDGE>(sw, ps, c, iter, on_edge);
  wave_sync();
  PHASE(5);
  // ---- phase 4: per-view sampling probabilities with the 4-neighbour priors (DPE.cu:1552-1590)
  if (active) strong_view_probs(sw, ps, c, pc, B, center, iter);
  wave_sync();
  PHASE(6);
  // ---- samples + view weights (cooperative), then the selected-view list
  Rng rs;
  rng_init(rs, (uint32_t)center, pc.seed32, STREAM_ITER_BASE + 4 * iter + 0, pc.salt);
  view_sample_coop(sw.sp(ps), sw.sample_counts(ps), nv, c, C, active, rs, sw.vw(ps), B.vw + (size_t)center * DPE_MAX_IMAGES);
  PHASE(12);
  uint32_t tsv = 0; float wnorm = 0.0f;
  strong_selected_views<kSpread>(sw, ps, c, lane, active, rs, tsv, wnorm);
  wave_sync();
  PHASE(7);
  const int nsel = active ? sw.nsel(ps) : 0;
  // ---- phase 5: final costs of the 8 directions
  if (active && c < 8) strong_final_cost(sw, ps, c);
  wave_sync();
  PHASE(8);
  // ---- serial: propagation acceptance + refinement hypotheses (DPE.cu:1617-1654, 1065-1095)
  float cost_now = 0.0f, cost_written = 0.0f, depth_now = 0.0f;
  float4 pnow = make_float4(0, 0, 0, 0);
  // lanes 1..4 evaluate the refinement draws while lane 0 runs the acceptance; the hypotheses are
  // then finished from them
  if (active && c >= 1 && c <= 4) refine_draws_lane(rs, c, sw.rnd(ps));
  if (active && c == 0) {
    const float* fc = sw.fc(ps);
    int mi = 0; float mcost = fc[0];
    for (int i = 1; i < 8; ++i) if (fc[i] <= mcost) { mcost = fc[i]; mi = i; }
    const float4 curp = B.planes_snap[center];
    const float* cur_cost = sw.cost(ps) + C * nv;
    cost_now = sel_weighted_cost(sw.vw(ps), sw.sel_list(ps), nsel, wnorm, [&](int, int v) { return cur_cost[v]; });
    cost_written = cost_now;
    B.costs[center] = cost_now;
    depth_now = depth_from_plane(c0, curp, x, y);
    pnow = curp;
    const int f = sw.fin(ps)[mi];
    if (f >= 0) {
      const float4 cand = B.planes_snap[sw.pos(ps)[f]];
      if (accept_if_better(cand, depth_from_plane(c0, cand, x, y), fc[mi], dmin, dmax, depth_now, pnow, cost_now))
        B.sel[center] = tsv;
    }
  }
  wave_sync();
  if constexpr (kSpread) strong_hypotheses_spread(sw, ps, c, lane, active, pc, x, y, pnow, depth_now);
  else if (active && c == 0) refine_hypotheses(c0, x, y, dmin, dmax, pnow, depth_now, sw.rnd(ps), sw.hyp(ps));
  wave_sync();
  PHASE(9);
  // ---- phase 6: refinement NCCs, one flat pool of (pixel, hypothesis, selected view)
  {
    int cnt[P];
#pragma unroll
    for (int q = 0; q < P; ++q) cnt[q] = 5 * sw.nsel(q);
    POOL_STAT(1, [&] { int t = 0; for (int q = 0; q < P; ++q) t += cnt[q]; return t; }());
    int q, r;
    // a last round of at most kTailMaxJobs jobs is split by patch rows, as in the cost-vector pool
    // (whose LDS tail region is free again here)
    int total = 0;
#pragma unroll
    for (int p = 0; p < P; ++p) total += cnt[p];
    const int tail = total & 63;
    const bool split = kWideTails && fast && tail > 0 && tail <= kTailMaxJobs;
    if (tail > 0) TAIL_STAT(1, split ? tail_lanes_per_job(tail) : 1);
    const int jend = split ? total - tail : total;
    // refinement job (q, r): hypothesis r % 5 in the pixel's selected view r / 5 (the 5 hypotheses of
    // one view adjacent)
    auto ref_job = [&]() {
      const int h = r % 5, k = r / 5;
      const int cq = list[wbase + q];
      return TailJob{sw.patch(q), sw.sums(q), sw.ref(q) + h * nv + k, cq % W, cq / W, sw.sel_list(q)[k] + 1, sw.hyp(q)[h]};
    };
    for (int j = lane; j < jend && job_decode<P>(cnt, j, q, r); j += 64) {
      const TailJob J = ref_job();
      *J.out = ncc_old_any<U8>(fast, J.pw, J.sm[0], J.sm[1], J.sm[2], J.qx, J.qy, pc, B, J.v, J.pl);
    }
    if (split)
      pool_tail_split<U8>(tail, lane, sw.tail(), pc, B, [&](int t) { job_decode<P>(cnt, jend + t, q, r); return ref_job(); });
  }
  wave_sync();
  PHASE(10);
  // ---- hypothesis costs and depths (one lane each), then sequential acceptance + write-back on
  // lane 0 (DPE.cu:1097-1117, 1656-1665)
  if (active && c < 5) {
    const float* ref = sw.ref(ps) + c * nv;
    sw.fc(ps)[c] = sel_weighted_cost(sw.vw(ps), sw.sel_list(ps), nsel, sw.wnorm(ps), [&](int k, int) { return ref[k]; });
    sw.set_depth(ps, c, depth_from_plane(c0, sw.hyp(ps)[c], x, y));
  }
  wave_sync();
  PHASE(13);
  if (active && c == 0) {
    for (int h = 0; h < 5; ++h) accept_if_better(sw.hyp(ps)[h], sw.depth(ps, h), sw.fc(ps)[h], dmin, dmax, depth_now, pnow, cost_now);
    if (pc.P.state == DPE_REFINE_INIT) {
      if ((double)cost_now < (double)cost_written - 0.1) { B.costs[center] = cost_now; B.planes[center] = pnow; }
    } else {
      B.costs[center] = cost_now;
      B.planes[center] = pnow;
    }
  }
  PHASE(11);
  PHASE_END(0);
}

// ------------------------------------------------------------------------------ weak sweep
// The NCC-New cost of a weak pixel (DPE.cu:557-690) is 9 bilateral patches (its own, radius from
// the RANSAC radius map, and one around each deformable strong neighbour).  All tap weights are
// plane- and view-independent, so they are tabulated once per pixel in LDS together with the
// reference sums of each patch; an NCC job is then projection + bilinear fetch + 3 FMAs per tap.
struct WeakTab {
  const float* tc;                        // centre patch (w, w*grey) pairs [n_c^2][2]
  const float* tn;                        // neighbour k=1..8: pairs at [((k-1)*9 + t)*2]
  const float* sums;                      // [9][3]: ncc_pre (1/s_w, s_ref/s_w, var_ref) of each tabulated patch
  const short2* nbl;                      // [9] neighbour pixels (nb[0] = the pixel itself)
  const uint32_t* nsv;                    // [9] selected_views of the neighbours
  int rad_c, inc_c, n_c, rad_n, inc_n, n_n;
  bool tab_c, tab_n;
  float rc;                               // grey level of the pixel
  bool nb3;                               // neighbour patches are tabulated 3x3 and nbox is set
  float nbox[4];                          // x0, x1, y0, y1 of the union of the neighbour patches
};

// patch NCC with tabulated weights; the same tap order and arithmetic as patch_ncc_generic.
// NN > 0: the patch side n is the compile-time NN, so the tap loop unrolls and the gathers of a
// patch are in flight together (the weak sweep's patches are 3x3 and 4..6 square).
template <int U8, bool FAST, int NN = 0>
DEV void tab_taps(const PassConst& pc, const DevBufs& B, int v, const Homog& H0, int cx, int cy, int rad, int inc,
                  int n_rt, const float* __restrict__ tw, float* acc) {
  const int W = pc.W, Hh = pc.H;
  const Homog H = scale_cols(H0);
  const int n = NN > 0 ? NN : n_rt;
  const f2v* wp = (const f2v*)tw;            // (w, w*grey) pairs
  if constexpr (U8 != TEX_F32 && FAST) {
    const uint32_t stride = tex_stride<U8>(W), vadj = tap_vadj<U8>((uint32_t)v * tex_view<U8>(B), stride), coef = tap_coef<U8>(stride);
    const f2v tmax = tex_tmax2(W, Hh);
    f2v s_sr = f2s(0.0f);
    float s_ss = 0;
#pragma unroll
    for (int a = 0; a < (NN > 0 ? NN : n); ++a) {
      const float xf = (float)(cx - rad + a * inc);
      const f2v bxy = fma2((f2v){H.h[0], H.h[3]}, f2s(xf), (f2v){H.h[2], H.h[5]}) * f2s(kTexUnit);
      const float bz = __builtin_fmaf(H.h[6], xf, H.h[8]);
      f2v r_sr = f2s(0.0f);
      float r_ss = 0;
#pragma unroll
      for (int b = 0; b < (NN > 0 ? NN : n); ++b) {
        const float sp = tap_u8_fast<U8>(B, vadj, coef, tmax, H.h, bxy, bz, (float)(cy - rad + b * inc));
        const f2v w = wp[a * n + b];
        r_sr = fma2(w, f2s(sp), r_sr);
        const float ws = w.x * sp;
        r_ss = __builtin_fmaf(ws, sp, r_ss);
      }
      s_sr += r_sr; s_ss += r_ss;
    }
    acc[0] = s_sr.x; acc[1] = s_ss; acc[2] = s_sr.y;
  } else {
    float s_src = 0, s_ss = 0, s_rs = 0;
    for (int a = 0; a < n; ++a) {
      const float xf = (float)(cx - rad + a * inc);
      const float bx = __builtin_fmaf(H.h[0], xf, H.h[2]) * kTexUnit;
      const float by = __builtin_fmaf(H.h[3], xf, H.h[5]) * kTexUnit;
      const float bz = __builtin_fmaf(H.h[6], xf, H.h[8]);
      float r_src = 0, r_ss = 0, r_rs = 0;
      for (int b = 0; b < n; ++b) {
        const float yf = (float)(cy - rad + b * inc);
        const float qx = __builtin_fmaf(H.h[1], yf, bx);
        const float qy = __builtin_fmaf(H.h[4], yf, by);
        const float iz = rcp_tap<FAST>(__builtin_fmaf(H.h[7], yf, bz));
        const float sp = sample_src<U8>(B, v, W, Hh, qx, qy, iz);
        const f2v w = wp[a * n + b];
        r_src = __builtin_fmaf(w.x, sp, r_src);
        const float ws = w.x * sp;
        r_ss = __builtin_fmaf(ws, sp, r_ss);
        r_rs = __builtin_fmaf(w.y, sp, r_rs);
      }
      s_src += r_src; s_ss += r_ss; s_rs += r_rs;
    }
    acc[0] = s_src; acc[1] = s_ss; acc[2] = s_rs;
  }
}
// NMAX: the largest side the caller can pass (the neighbour patches are tabulated only up to 3)
template <int U8, int NMAX = 6>
DEV float patch_ncc_tab(const PassConst& pc, const DevBufs& B, int v, const Homog& H, int cx, int cy, int rad, int inc,
                        int n, const float* __restrict__ tw, const float* sm) {
  float a[3];
  if (rcp_range_ok(H, (float)(cx - rad), (float)(cx + rad), (float)(cy - rad), (float)(cy + rad))) {
    switch (n) {
      case 3: tab_taps<U8, true, 3>(pc, B, v, H, cx, cy, rad, inc, n, tw, a); break;
      case 4: tab_taps<U8, true, 4>(pc, B, v, H, cx, cy, rad, inc, n, tw, a); break;
      case 5: tab_taps<U8, true, 5>(pc, B, v, H, cx, cy, rad, inc, n, tw, a); break;
      case 6: tab_taps<U8, true, 6>(pc, B, v, H, cx, cy, rad, inc, n, tw, a); break;
      default: tab_taps<U8, true>(pc, B, v, H, cx, cy, rad, inc, n, tw, a); break;
    }
  } else {
    tab_taps<U8, false>(pc, B, v, H, cx, cy, rad, inc, n, tw, a);
  }
  count_work(B, 0, (unsigned long long)(n * n));
  return ncc_finalize_pre(sm[0], sm[1], sm[2], a[0], a[1], a[2]);
}

// Weak-sweep path statistics (DPE_DIAG & 4; tools/weak_stats.py): per NCC-New,
// the centre patch side and path, the neighbour-patch paths, and per wave the number of distinct
// centre-patch variants its lanes execute one after another.  Off in the product.
#if DPE_WEAK_STATS
// 0 jobs, 1 centre outside, 2..11 n_c histogram (n 0..9, 9 = larger), 12 centre generic (untabulated),
// 13 centre tabulated but slow reciprocal, 14 neighbour box fast, 15 neighbour patches, 16 neighbour
// generic, 17 sum of distinct centre variants per wave call, 18 wave calls, 19 active lanes per wave call
static __device__ unsigned long long g_wstat[24];
DEV void wstat(int k, unsigned long long n = 1) { atomicAdd(&g_wstat[k], n); }
DEV void wstat_variants(int variant) {
  uint64_t rem = __ballot(1);
  const int first = __builtin_ctzll(rem);
  const unsigned long long act = __popcll(rem);
  unsigned long long nv = 0;
  while (rem) {
    const int l = __builtin_ctzll(rem);
    const int V = __shfl(variant, l);
    rem &= ~__ballot(variant == V);
    ++nv;
  }
  if ((int)(threadIdx.x & 63) == first) { wstat(17, nv); wstat(18); wstat(19, act); }
}
#define WSTAT(...) wstat(__VA_ARGS__)
#else
#define WSTAT(...) do {} while (0)
#endif

// ComputeBilateralNCCNew (DPE.cu:557-690) of the tabulated weak pixel (px, py)
template <int U8>
DEV float ncc_new_tab(const PassConst& pc, const DevBufs& B, const WeakTab& T, int px, int py, int v, const float4& pl) {
  const int W = pc.W, Hh = pc.H;
  const Homog H = make_homography(pc, v, pl);
  count_work(B, 1, 0);
  WSTAT(0);
  if (center_outside(pc, v, H, px, py)) { WSTAT(1); return 2.0f; }
  float center_cost = 0.0f, strong_cost = 0.0f;
  int strong_count = 0;
  {   // k = 0: the pixel's own patch
    const short2 np = T.nbl[0];
    if (!(np.x == -1 || np.y == -1)) {
      const float2 nsp = project_h(H, (float)np.x, (float)np.y);
      if (nsp.x < 0 || nsp.y < 0 || nsp.x >= (float)W || nsp.y >= (float)Hh) return 2.0f;
#if DPE_WEAK_STATS
      WSTAT(2 + min(T.n_c, 9));
      if (!T.tab_c) WSTAT(12);
      else if (!rcp_range_ok(H, (float)(np.x - T.rad_c), (float)(np.x + T.rad_c), (float)(np.y - T.rad_c), (float)(np.y + T.rad_c))) WSTAT(13);
      wstat_variants(T.tab_c ? T.n_c : 100 + T.n_c);
#endif
      center_cost = T.tab_c ? patch_ncc_tab<U8>(pc, B, v, H, np.x, np.y, T.rad_c, T.inc_c, T.n_c, T.tc, T.sums)
                            : patch_ncc_generic<U8>(pc, B, v, H, np.x, np.y, T.rc, T.rad_c, T.inc_c);
    }
  }
  // k = 1..8; one range check over the union of the 3x3 neighbour patches selects the fast
  // reciprocal for all of them (it is exact on every tap inside that box)
  const bool nfast = T.nb3 && rcp_range_ok(H, T.nbox[0], T.nbox[1], T.nbox[2], T.nbox[3]);
  if (nfast) WSTAT(14);
#pragma unroll 1
  for (int k = 1; k < DPE_NEIGHBOUR_NUM; ++k) {
    const short2 np = T.nbl[k];
    if (np.x == -1 || np.y == -1) continue;
    const float2 nsp = nfast ? project_h_fast(H, (float)np.x, (float)np.y) : project_h(H, (float)np.x, (float)np.y);
    if (nsp.x < 0 || nsp.y < 0 || nsp.x >= (float)W || nsp.y >= (float)Hh) {
      if (isSet(T.nsv[k], v - 1)) { strong_cost += 2.0f; strong_count++; }
      continue;
    }
    float tc;
    WSTAT(15);
    if (!nfast && !T.tab_n) WSTAT(16);
    if (nfast) {
      float a[3];
      tab_taps<U8, true, 3>(pc, B, v, H, np.x, np.y, T.rad_n, T.inc_n, 3, T.tn + (k - 1) * 18, a);
      count_work(B, 0, 9ull);
      const float* sm = T.sums + 3 * k;
      tc = ncc_finalize_pre(sm[0], sm[1], sm[2], a[0], a[1], a[2]);
    } else {
      tc = T.tab_n ? patch_ncc_tab<U8, 6>(pc, B, v, H, np.x, np.y, T.rad_n, T.inc_n, T.n_n, T.tn + (k - 1) * 18,
                                       T.sums + 3 * k)
                   : patch_ncc_generic<U8>(pc, B, v, H, np.x, np.y, T.rc, T.rad_n, T.inc_n);
    }
    strong_cost += tc; strong_count++;
  }
  if (strong_count == 0) return center_cost;
  strong_cost /= (float)strong_count;
  strong_cost = MINo(strong_cost, 2.0f);
  return (float)(0.25 * (double)center_cost + 0.75 * (double)strong_cost);
}

// LDS floats per weak pixel (lds_layout.h WeakCarve: fixed part, then [8][nv] costs, [nv] sampling
// probabilities, [nv] selected views, [7][nv] hypothesis values; multiple of 4).  At 9 source views a
// pixel takes 640 floats, so four 4-wave workgroups (4 x 40 KB, the whole budget) fit a CU's LDS.
using WC = lds::WeakCarve;
constexpr int kWeakFixed = WC::FIXED;
__host__ __device__ inline int weak_lds_per_pixel(int nv) { return WC::per_pixel(nv); }
// The patch geometries of a weak pixel: the centre patch's radius is the pixel's (RANSAC radius map),
// the neighbour patches' the pass's; n = the side in taps.  A patch of side <= 6 (centre) or <= 3
// (neighbours) is tabulated; rc = the pixel's grey level, the bilateral weights' centre.
struct WeakSides {
  int rad_c, inc_c, n_c, rad_n, inc_n, n_n;
  bool tab_c, tab_n;
  float rc;
  // phase 1 by patch rows (the common case: centre side <= 6, 3x3 neighbour patches)
  DEV bool by_rows() const { return tab_c && tab_n && n_n == 3; }
};
// A pixel's block of that carve: typed pointers to its regions, for the lane's own pixel and, in the
// pooled phases, for any pixel of the workgroup.  Holds the block's base and nv, nothing else.
struct WeakPixel {
  float* b;
  int nv;
  DEV float* pw() const { return b + WC::PW; }                                   // [108] Old-NCC patch (patch_lds_build)
  DEV float* tc() const { return b + WC::TC; }                                   // centre patch table, pairs [36][2]
  DEV float* tn() const { return b + WC::TN; }                                   // neighbour patch tables, pairs [8][9][2]
  DEV float* sums() const { return b + WC::SUMS; }                               // [9][3] ncc_pre of each tabulated patch
  DEV float* osum() const { return b + WC::OSUM; }                               // [3] Old-NCC patch sums
  DEV float4* cpl() const { return (float4*)(b + WC::CPL); }                     // [8] candidate planes
  DEV float4* hyp() const { return (float4*)(b + WC::HYP); }                     // [5] hypotheses, then:
  DEV float4& final_plane() const { return hyp()[5]; }
  DEV float4& fit_plane() const { return hyp()[6]; }
  DEV float* rsum(int row) const { return b + WC::RSUM + 3 * row; }              // phases 1-1b: row sums of the centre patch
  DEV float* fc() const { return b + WC::FC; }                                   // [8] final candidate costs
  DEV int* misc() const { return (int*)(b + WC::MISC); }                         // WC::M_* slots
  DEV int* flags() const { return misc() + WC::M_FLAGS; }                        // [8] neighbour i + 1 is strong: a candidate
  DEV short2* nbl() const { return (short2*)(b + WC::NBL); }                     // [9] neighbour pixels ([0] = the pixel itself)
  DEV uint32_t* nsv() const { return (uint32_t*)(b + WC::NSV); }                 // [9] selected views of the neighbours
  DEV int* alias() const { return (int*)(b + WC::ALIAS); }                       // [8] earlier row with a bitwise-identical plane
  DEV uint8_t* vwl() const { return (uint8_t*)(b + WC::VWL); }                   // [32] view weights
  DEV float* rnd() const { return b + WC::RND; }                                 // [12] refinement draws (over alias)
  DEV float* cost() const { return b + WC::cost(nv); }                           // [8][nv]
  DEV float* sp() const { return b + WC::sp(nv); }                               // [nv]
  DEV int* sel_list() const { return (int*)(b + WC::sel(nv)); }                  // [nv]
  DEV float* hv(int row) const { return b + WC::hv(nv) + row * nv; }             // [7][nv] plane x selected-view values
  DEV int* sample_counts() const { return (int*)hv(0); }                         // [nv] view_sample_coop's counts (over hv)
  DEV int& nsel() const { return misc()[WC::M_NSEL]; }
  DEV int& pool_jobs() const { return misc()[WC::M_POOL]; }                      // the pixel's jobs in the next pool
  DEV int& cmask() const { return misc()[WC::M_CMASK]; }                         // candidates with a cost vector of their own
  DEV float wnorm() const { return __int_as_float(misc()[WC::M_WNORM]); }
  DEV void set_wnorm(float w) const { misc()[WC::M_WNORM] = __float_as_int(w); }
  // the header the pooled phases read: the centre patch's geometry, the grey level, the box of the
  // neighbour patches (nb3: they are tabulated 3x3 and the box is set)
  DEV void set_header(int rad_c, int inc_c, int n_c, bool nb3, const float* nbox, float rc) const {
    misc()[WC::M_RADC] = rad_c; misc()[WC::M_INCC] = inc_c; misc()[WC::M_NC] = n_c; misc()[WC::M_NB3] = nb3 ? 1 : 0;
    b[WC::NBOX_A] = nbox[0]; b[WC::NBOX_A + 1] = nbox[1]; b[WC::NBOX_A + 2] = nbox[2]; b[WC::NBOX_B] = nbox[3];
    b[WC::RC] = rc;
  }
  // the tables of the pixel as ncc_new_tab takes them; the neighbour patches' geometry is the pass's,
  // so any pixel's `g` serves
  DEV WeakTab tab(const WeakSides& g) const {
    const int* h = misc();
    WeakTab t;
    t.rad_c = h[WC::M_RADC]; t.inc_c = h[WC::M_INCC]; t.n_c = h[WC::M_NC]; t.nb3 = h[WC::M_NB3] != 0;
    t.rad_n = g.rad_n; t.inc_n = g.inc_n; t.n_n = g.n_n; t.tab_n = g.tab_n;
    t.tab_c = t.n_c >= 1 && t.n_c <= 6;
    t.rc = b[WC::RC];
    t.nbox[0] = b[WC::NBOX_A]; t.nbox[1] = b[WC::NBOX_A + 1]; t.nbox[2] = b[WC::NBOX_A + 2]; t.nbox[3] = b[WC::NBOX_B];
    t.tc = tc(); t.tn = tn(); t.sums = sums();
    t.nbl = nbl(); t.nsv = nsv();
    return t;
  }
};

// ---- the weak sweep's per-pixel phases (no barrier inside: k_weak_coop puts one after each)
// phase 1, by_rows(): the tables by patch rows with their reference sums (the order of
// weak_table_sums): lanes 0..n_c-1 a centre row each (row sums to rsum, added in row order by
// weak_centre_sums), lanes 8..15 a 3x3 neighbour patch each (sums complete); a lane's texel loads
// are issued together
DEV void weak_tables_by_rows(const WeakPixel& me, int c, const PassConst& pc, const DevBufs& B, const short2* nbg,
                             const WeakSides& g) {
  const int W = pc.W, Hh = pc.H;
  const float ss = pc.P.sigma_spatial, sc = pc.P.sigma_color;
  const int rad_c = g.rad_c, inc_c = g.inc_c, n_c = g.n_c, rad_n = g.rad_n, inc_n = g.inc_n;
  if (c < n_c) {
    const short2 np = nbg[0];
    if (!(np.x == -1 || np.y == -1)) {
      const int i = -rad_c + c * inc_c;
      float rp[6];
#pragma unroll
      for (int b = 0; b < 6; ++b) rp[b] = b < n_c ? ref_texel(B.ref, W, Hh, np.x + i, np.y - rad_c + b * inc_c) : 0.0f;
      float* tcp = me.tc();
      float r_ref = 0, r_rr = 0, r_w = 0;
#pragma unroll
      for (int b = 0; b < 6; ++b) {
        if (b >= n_c) break;
        const float w = bilateral_weight(i, -rad_c + b * inc_c, rp[b], g.rc, ss, sc);
        const float wr = w * rp[b];
        tcp[2 * (c * n_c + b)] = w; tcp[2 * (c * n_c + b) + 1] = wr;
        r_ref = r_ref + wr;
        r_rr = __builtin_fmaf(wr, rp[b], r_rr);
        r_w = r_w + w;
      }
      float* rs3 = me.rsum(c);
      rs3[0] = r_ref; rs3[1] = r_rr; rs3[2] = r_w;
    }
  } else if (c >= 8) {
    const int k = c - 7;
    const short2 np = nbg[k];
    if (!(np.x == -1 || np.y == -1)) {
      float rp[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) rp[t] = ref_texel(B.ref, W, Hh, np.x - rad_n + (t / 3) * inc_n, np.y - rad_n + (t % 3) * inc_n);
      float* tp = me.tn() + (k - 1) * 18;
      float a_ref = 0, a_rr = 0, a_w = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        float r_ref = 0, r_rr = 0, r_w = 0;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          const float w = bilateral_weight(-rad_n + a * inc_n, -rad_n + b * inc_n, rp[a * 3 + b], g.rc, ss, sc);
          const float wr = w * rp[a * 3 + b];
          tp[2 * (a * 3 + b)] = w; tp[2 * (a * 3 + b) + 1] = wr;
          r_ref = r_ref + wr;
          r_rr = __builtin_fmaf(wr, rp[a * 3 + b], r_rr);
          r_w = r_w + w;
        }
        a_ref += r_ref; a_rr += r_rr; a_w += r_w;
      }
      float* sm = me.sums() + 3 * k;
      ncc_pre(a_ref, a_rr, a_w, sm[0], sm[1], sm[2]);
    }
  }
}
// phase 1 otherwise: the taps of the tabulated patches dealt over the pixel's C lanes
DEV void weak_tables_by_taps(const WeakPixel& me, int c, int C, const PassConst& pc, const DevBufs& B, const short2* nbg,
                             const WeakSides& g) {
  const float ss = pc.P.sigma_spatial, sc = pc.P.sigma_color;
  const int rad_c = g.rad_c, inc_c = g.inc_c, n_c = g.n_c, rad_n = g.rad_n, inc_n = g.inc_n, n_n = g.n_n;
  const int ntc = g.tab_c ? n_c * n_c : 0, ntn = g.tab_n ? n_n * n_n : 0;
  for (int t = c; t < ntc + 8 * ntn; t += C) {
    int k, tt, n, rad, inc;
    if (t < ntc) { k = 0; tt = t; n = n_c; rad = rad_c; inc = inc_c; }
    else { k = 1 + (t - ntc) / ntn; tt = (t - ntc) % ntn; n = n_n; rad = rad_n; inc = inc_n; }
    const short2 np = nbg[k];
    if (np.x == -1 || np.y == -1) continue;
    const int i = -rad + (tt / n) * inc, j = -rad + (tt % n) * inc;
    const float rp = ref_texel(B.ref, pc.W, pc.H, np.x + i, np.y + j);
    const float w = bilateral_weight(i, j, rp, g.rc, ss, sc);
    float* dst = k == 0 ? me.tc() + 2 * tt : me.tn() + 2 * ((k - 1) * 9 + tt);
    dst[0] = w; dst[1] = w * rp;
  }
}
// phase 1: the neighbours with their selected views
DEV void weak_neighbours(const WeakPixel& me, int c, int C, const PassConst& pc, const DevBufs& B, const short2* nbg) {
  for (int k = c; k < 9; k += C) {
    const short2 np = nbg[k];
    me.nbl()[k] = np;
    me.nsv()[k] = (np.x == -1 || np.y == -1) ? 0u : B.sel[np.x + np.y * pc.W];
  }
}
// phase 1: the candidate rows: neighbour i + 1 is a candidate if it is strong (its plane to cpl),
// otherwise its cost row is the reference's zero row
DEV void weak_candidate_rows(const WeakPixel& me, int c, int C, const PassConst& pc, const DevBufs& B, const short2* nbg) {
  const int W = pc.W, nv = me.nv;
  for (int i = c; i < 8; i += C) {
    const short2 np = nbg[i + 1];
    const bool fl = !(np.x == -1 || np.y == -1) && B.weak[np.x + np.y * W] == DPE_STRONG;
    me.flags()[i] = fl ? 1 : 0;
    if (fl) me.cpl()[i] = B.planes[np.x + np.y * W];
    else for (int v = 0; v < nv; ++v) me.cost()[i * nv + v] = (i == 0 && v == 0) ? 2.0f : 0.0f;
  }
}
// phase 1b, one lane: the header, with the union box of the neighbour patches (k = 1..8) for the
// one-check fast path of ncc_new_tab
DEV void weak_header(const WeakPixel& me, const WeakSides& g) {
  const int rad_n = g.rad_n;
  bool nb3 = false;
  float nbox[4];
  if (g.tab_n && g.n_n == 3) {
    int x0 = 0x7FFFFFFF, x1 = -0x7FFFFFFF, y0 = 0x7FFFFFFF, y1 = -0x7FFFFFFF;
    for (int k = 1; k < DPE_NEIGHBOUR_NUM; ++k) {
      const short2 np = me.nbl()[k];
      if (np.x == -1 || np.y == -1) continue;
      x0 = min(x0, (int)np.x); x1 = max(x1, (int)np.x); y0 = min(y0, (int)np.y); y1 = max(y1, (int)np.y);
    }
    if (x0 <= x1) {
      nb3 = true;
      nbox[0] = (float)(x0 - rad_n); nbox[1] = (float)(x1 + rad_n);
      nbox[2] = (float)(y0 - rad_n); nbox[3] = (float)(y1 + rad_n);
    }
  }
  me.set_header(g.rad_c, g.inc_c, g.n_c, nb3, nbox, g.rc);
}
// phase 1b, by_rows(), one lane: the centre patch's row sums added in row order
DEV void weak_centre_sums(const WeakPixel& me, int n_c) {
  const short2 np = me.nbl()[0];
  if (np.x == -1 || np.y == -1) return;
  float a_ref = 0, a_rr = 0, a_w = 0;
  for (int a = 0; a < n_c; ++a) {
    const float* rs3 = me.rsum(a);
    a_ref += rs3[0]; a_rr += rs3[1]; a_w += rs3[2];
  }
  float* sm = me.sums();
  ncc_pre(a_ref, a_rr, a_w, sm[0], sm[1], sm[2]);
}
// phase 1b otherwise: the reference sums of every tabulated patch (tap order of patch_ncc_generic),
// one patch per lane
DEV void weak_table_sums(const WeakPixel& me, int c, int C, const PassConst& pc, const DevBufs& B, const WeakSides& g) {
  const int rad_c = g.rad_c, inc_c = g.inc_c, n_c = g.n_c, rad_n = g.rad_n, inc_n = g.inc_n, n_n = g.n_n;
  const bool tab_c = g.tab_c, tab_n = g.tab_n;
  for (int k = c; k < 9; k += C) {
    const short2 np = me.nbl()[k];
    if (np.x == -1 || np.y == -1 || !(k == 0 ? tab_c : tab_n)) continue;
    const int n = k == 0 ? n_c : n_n, rad = k == 0 ? rad_c : rad_n, inc = k == 0 ? inc_c : inc_n;
    const float* tp = k == 0 ? me.tc() : me.tn() + (k - 1) * 18;
    float a_ref = 0, a_rr = 0, a_w = 0;
    for (int a = 0; a < n; ++a) {
      float r_ref = 0, r_rr = 0, r_w = 0;
      for (int b = 0; b < n; ++b) {
        const float rp = ref_texel(B.ref, pc.W, pc.H, np.x - rad + a * inc, np.y - rad + b * inc);
        const float w = tp[2 * (a * n + b)], wr = tp[2 * (a * n + b) + 1];
        r_ref = r_ref + wr;
        r_rr = __builtin_fmaf(wr, rp, r_rr);
        r_w = r_w + w;
      }
      a_ref += r_ref; a_rr += r_rr; a_w += r_w;
    }
    float* sm = me.sums() + 3 * k;
    ncc_pre(a_ref, a_rr, a_w, sm[0], sm[1], sm[2]);
  }
}
// phase 1b: bitwise-identical neighbour planes share one cost vector: alias = first earlier flagged
// row with the same plane (lanes 8..15; lanes 0..8 build the sums)
DEV void weak_alias_rows(const WeakPixel& me, int c, int C) {
  for (int i = c - 8; i >= 0 && i < 8; i += C) {
    int a = i;
    if (me.flags()[i]) {
      const float4 pl = me.cpl()[i];
      for (int t = 0; t < i; ++t)
        if (me.flags()[t] && same_plane_bits(me.cpl()[t], pl)) { a = t; break; }
    }
    me.alias()[i] = a;
  }
}
// phase 3: per-view probabilities with the deformable-neighbour priors (DPE.cu:1768-1790)
DEV void weak_view_probs(const WeakPixel& me, int c, int C, int iter) {
  const int nv = me.nv;
  const float* cost = me.cost();
  const float cost_threshold = (float)(0.8 * (double)d_expf((float)(iter * iter) / (-90.0f)));
  auto cst = [&](int j, int i) -> float { return cost[j * nv + i]; };
  for (int v = c; v < nv; v += C) {
    float prior = 0.0f;
    for (int i = 0; i < 8; ++i) {
      const short2 np = me.nbl()[i + 1];
      if (np.x == -1 || np.y == -1) continue;
      prior += isSet(me.nsv()[i + 1], v) == 1 ? 0.9f : 0.1f;
    }
    me.sp()[v] = view_prob_raw(cst, v, cost_threshold) * prior;
  }
}
// the final cost of candidate i over the sampled views, with the geometric term (DPE.cu:1792-1810)
DEV void weak_final_cost(const WeakPixel& me, int i, const PassConst& pc, const DevBufs& B, int x, int y, float wn) {
  const int nv = me.nv;
  const bool geom = pc.P.geom_consistency;
  const float gf = pc.P.geom_factor;
  const float* cost = me.cost();
  const uint8_t* vwl = me.vwl();
  const bool fl = me.flags()[i] != 0;
  const float3 fwi = (geom && fl) ? geom_point(pc, x, y, me.cpl()[i]) : make_float3(0.0f, 0.0f, 0.0f);
  float f = 0.0f;
  for (int j = 0; j < nv; ++j) {
    const int w = vwl[j];
    if (w > 0) {
      if (geom) {
        if (fl) f += w * (cost[i * nv + j] + gf * geom_cost_at(pc, B, x, y, j + 1, fwi));
        else f += w * (cost[i * nv + j] + gf * 3.0f);
      } else {
        f += w * cost[i * nv + j];
      }
    }
  }
  me.fc()[i] = f / wn;
}

// CheckerboardPropagationWeak (DPE.cu:1668-1862) + PlaneHypothesisRefinementWeak (:1120-1212).
// C = 16 lanes per pixel, 4 pixels per wave, blockDim.x/64 waves per workgroup.
//
// Pooled phases: the NCCs of all the workgroup's pixels are dealt round-robin over its lanes, so a
// job carries its pixel q (0..npx-1, the workgroup's pixels in list order) and pix(q) is that pixel's
// LDS block.  A pool's jobs fill whole waves first, so a wave with no job left skips the round and
// its SIMD issues other waves (pools over one wave's 4 pixels left 27-46 of 64 lanes idle in the
// current-plane, refinement and final-cost rounds).  Each pixel's job count sits in its pool_jobs();
// a job index is decoded by a scan over the pool's pixels.  The barriers around a pool are
// workgroup-wide.
template <int U8, int C>
__global__ void __launch_bounds__(256, kTapWaves) k_weak_coop(const PassConst* __restrict__ pcp, DevBufs B, int iter,
                                                   const int* __restrict__ list, const int* __restrict__ nlist_p) {
  extern __shared__ float4 lds4[];
  // (a local: with `(float*)lds4` written into pix() below, the first job pool of every instantiation
  // grows by 240 instructions, scalar values kept in VGPR lanes and their wait states, and the weak
  // class by 0.2 ms per pass; profiles/sweep_cleanup_ab.md)
  float* lds = (float*)lds4;
  static_assert(C == 16, "the per-pixel phases give lanes 0..8 the patch sums and lanes 8..15 the alias rows");
  constexpr int P = 64 / C;
  const PassConst& pc = *pcp;
  const int nlist = *nlist_p;
  const int wpb = blockDim.x >> 6;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ps = lane / C, c = lane % C;
  const int W = pc.W, Hh = pc.H, nv = pc.N - 1;
  const DpeCamera& c0 = pc.cams[0];
  const int wgbase = xcd_remap(blockIdx.x, gridDim.x, B.xcd_rows * 16) * wpb * P;   // list index of the pool's pixel 0
  if (wgbase >= nlist) return;                           // workgroup-uniform tail
  const int gi = wgbase + wave * P + ps;
  const bool active = gi < nlist;
  const int center = active ? list[gi] : 0;
  const int x = center % W, y = center / W;
  // the LDS carve (lds_layout.h WeakCarve): one block per pixel, `me` the lane's own
  const int S = weak_lds_per_pixel(nv);
  auto pix = [&](int q) { return WeakPixel{lds + (size_t)q * S, nv}; };
  const WeakPixel me = pix(wave * P + ps);
  const int npx = wpb * P;

  const bool geom = pc.P.geom_consistency;
  const float gf = pc.P.geom_factor;
  const bool fast_old = pc.P.strong_radius == 5 && pc.P.strong_increment == 2;
  WeakSides g;
  g.rad_c = pc.P.strong_radius; g.inc_c = pc.P.strong_increment;
  if (pc.P.use_radius && active) { g.rad_c = B.radius[center]; g.inc_c = MAXo(2, d2i(2.0 * g.rad_c / 5.0)); }
  g.rad_n = pc.P.weak_radius; g.inc_n = pc.P.weak_increment;
  g.n_c = g.rad_c >= 0 ? (2 * g.rad_c) / g.inc_c + 1 : 0;
  g.n_n = g.rad_n >= 0 ? (2 * g.rad_n) / g.inc_n + 1 : 0;
  g.tab_c = g.n_c >= 1 && g.n_c <= 6;
  g.tab_n = g.n_n >= 1 && g.n_n <= 3;
  g.rc = active ? ref_texel(B.ref, W, Hh, x, y) : 0.0f;
  const short2* nbg = B.nb + (size_t)center * 9;
  auto pool_total = [&]() -> int { int t = 0; for (int q = 0; q < npx; ++q) t += pix(q).pool_jobs(); return t; };
  auto pool_decode = [&](int j, int& q, int& r) { q = 0; for (int cc; j >= (cc = pix(q).pool_jobs()); ++q) j -= cc; r = j; };
  auto pool_stat_g = [&](int k, int jobs) {   // DPE_DIAG & 16: jobs, wave rounds with a job, waves
#if DPE_POOL_STATS
    if (threadIdx.x == 0) {
      atomicAdd(&g_pool[k][0], (unsigned long long)jobs);
      atomicAdd(&g_pool[k][1], (unsigned long long)((jobs + 63) / 64));
      atomicAdd(&g_pool[k][2], (unsigned long long)(blockDim.x / 64));
    }
#else
    (void)k; (void)jobs;
#endif
  };
  const bool rows1 = g.by_rows();

  PHASE_BEGIN();
  // ---- phase 1: neighbours, weight tables, Old-NCC patch, candidate rows
  if (active) {
    if (fast_old) patch_lds_build<C>(me.pw(), pc, B, x, y, c);
    weak_neighbours(me, c, C, pc, B, nbg);
    if (rows1) weak_tables_by_rows(me, c, pc, B, nbg, g);
    else weak_tables_by_taps(me, c, C, pc, B, nbg, g);
    weak_candidate_rows(me, c, C, pc, B, nbg);
  }
  wave_sync();
  PHASE(0);
  // ---- phase 1b: the header, the reference sums of every tabulated patch, the alias rows
  if (active) {
    if (c == C - 2) weak_header(me, g);
    if (!rows1) weak_table_sums(me, c, C, pc, B, g);
    else if (c == 0) weak_centre_sums(me, g.n_c);
    if (c == C - 1 && fast_old) { float* os = me.osum(); patch_lds_pre(me.pw(), os[0], os[1], os[2]); }
    weak_alias_rows(me, c, C);
  }
  wave_sync();
  PHASE(1);
  // ---- phase 2: candidate cost vectors, jobs (unique flagged neighbour plane, view)
  if (active && c == 0) {
    uint32_t um = 0;
    for (int i = 0; i < 8; ++i) if (me.flags()[i] && me.alias()[i] == i) um |= 1u << i;
    me.cmask() = (int)um;
    me.pool_jobs() = __builtin_popcount(um);
  }
  if (!active && c == 0) me.pool_jobs() = 0;
  __syncthreads();
  {
    const int Sj = pool_total();
    int q, r;
    pool_stat_g(2, Sj * nv);
    // view-major: the lanes of one round gather from the same source images
    for (int j = threadIdx.x; j < Sj * nv; j += blockDim.x) {
      pool_decode(j % Sj, q, r);
      const int v = j / Sj + 1;
      const WeakPixel px = pix(q);
      uint32_t m = (uint32_t)px.cmask();
      for (; r > 0; --r) m &= m - 1;
      const int i = __builtin_ctz(m);
      const int cq = list[wgbase + q];
      px.cost()[i * nv + v - 1] = ncc_new_tab<U8>(pc, B, px.tab(g), cq % W, cq / W, v, px.cpl()[i]);
    }
  }
  __syncthreads();
  PHASE(2);
  if (active)
    for (int i = c; i < 8; i += C)
      if (me.flags()[i] && me.alias()[i] != i)
        for (int v = 0; v < nv; ++v) me.cost()[i * nv + v] = me.cost()[me.alias()[i] * nv + v];
  wave_sync();
  PHASE(3);
  // ---- phase 3: per-view probabilities with the deformable-neighbour priors (DPE.cu:1768-1790)
  if (active) weak_view_probs(me, c, C, iter);
  wave_sync();
  PHASE(4);
  Rng rs;
  rng_init(rs, (uint32_t)center, pc.seed32, STREAM_ITER_BASE + 4 * iter + 2, pc.salt);
  view_sample_coop(me.sp(), me.sample_counts(), nv, c, C, active, rs, me.vwl(), B.vw + (size_t)center * DPE_MAX_IMAGES);
  uint32_t tsv = 0; float wnorm = 0.0f;
  if (active && c == 0) {
    rng_seek(rs, 15);
    int ns = 0;
    for (int i = 0; i < nv; ++i) if (me.vwl()[i] > 0) { setBit(tsv, i); wnorm += me.vwl()[i]; me.sel_list()[ns++] = i; }
    me.nsel() = ns;
    me.set_wnorm(wnorm);
    const float4 f6 = B.fit_plane[center];
    me.fit_plane() = f6;
    me.pool_jobs() = ((f6.x == 0 && f6.y == 0 && f6.z == 0) ? 1 : 2) * ns;   // current (+ fit) plane jobs
  }
  if (!active && c == 0) me.pool_jobs() = 0;
  __syncthreads();
  PHASE(5);
  const int nsel = active ? me.nsel() : 0;
  const float wn = active ? me.wnorm() : 1.0f;
  const float4 cur = active ? B.planes[center] : make_float4(0, 0, 0, 1);
  const float4 fp = active ? B.fit_plane[center] : make_float4(0, 0, 0, 0);
  const bool has_fit = !(fp.x == 0 && fp.y == 0 && fp.z == 0);
  // pixel q's hyp_cost term (DPE.cu:1140-1150) of plane pl in view v.  Its two pools below are two
  // loops: as one loop over a plane functor they cost the f32-texel kernel 16 B/lane of scratch.
  auto hyp_val_q = [&](const WeakPixel& px, int q, int v, const float4& pl) __attribute__((always_inline)) -> float {
    const int cq = list[wgbase + q];
    const int qx = cq % W, qy = cq / W;
    const float cn = ncc_new_tab<U8>(pc, B, px.tab(g), qx, qy, v, pl);
    return geom ? cn + gf * geom_cost(pc, B, qx, qy, v, pl) : cn;
  };
  // ---- phase 4: current plane and fit plane over the selected views; final candidate costs
  {
    const int tot = pool_total();
    pool_stat_g(3, tot);
    int q, r;
    for (int j = threadIdx.x; j < tot; j += blockDim.x) {
      pool_decode(j, q, r);
      const WeakPixel px = pix(q);
      const int ns = px.nsel();
      const int h = r / ns, k = r % ns;
      const int v = px.sel_list()[k] + 1;
      px.hv(h)[k] = hyp_val_q(px, q, v, h ? px.fit_plane() : B.planes[list[wgbase + q]]);
    }
  }
  PHASE(12);   // (phase 6 from here: the final candidate costs)
  if (active)
    for (int i = c; i < 8; i += C) weak_final_cost(me, i, pc, B, x, y, wn);
  __syncthreads();   // the current / fit-plane values of every pool pixel are in
  PHASE(6);
  // ---- serial: propagation acceptance, fit plane, refinement hypotheses (DPE.cu:1792-1843, 1120-1170)
  float cost_now = 0.0f, cost_written = 0.0f, depth_now = 0.0f;
  float4 pnow = cur;
  const float dmin = pc.P.depth_min, dmax = pc.P.depth_max;
  // the cost of the plane whose values are in row `row` of hv
  auto row_cost = [&](int row) {
    const float* hv = me.hv(row);
    return sel_weighted_cost(me.vwl(), me.sel_list(), nsel, wnorm, [&](int k, int) { return hv[k]; });
  };
  // lanes 1..4 evaluate the refinement draws while lane 0 runs the acceptance; lane 0 then finishes
  // the hypotheses from them
  if (active && has_fit && c >= 1 && c <= 4) refine_draws_lane(rs, c, me.rnd());
  if (active && c == 0) {
    const float* fc = me.fc();
    int mi = 0; float mcost = fc[0];
    for (int i = 1; i < 8; ++i) if (fc[i] <= mcost) { mcost = fc[i]; mi = i; }
    cost_now = row_cost(0);
    cost_written = cost_now;
    depth_now = depth_from_plane(c0, cur, x, y);
    if (me.flags()[mi]) {
      const float4 cand_pl = me.cpl()[mi];
      if (accept_if_better(cand_pl, depth_from_plane(c0, cand_pl, x, y), fc[mi], dmin, dmax, depth_now, pnow, cost_now))
        B.sel[center] = tsv;
    }
    if (has_fit) {
      const float tc = row_cost(1);
      accept_if_better(fp, depth_from_plane(c0, fp, x, y), tc, dmin, dmax, depth_now, pnow, cost_now);
    }
  }
  wave_sync();
  if (active && c == 0 && has_fit) refine_hypotheses(c0, x, y, dmin, dmax, pnow, depth_now, me.rnd(), me.hyp());
  if (c == 0) me.pool_jobs() = active && has_fit ? 5 * nsel : 0;
  __syncthreads();
  PHASE(7);
  // ---- phase 5: refinement NCCs, jobs (hypothesis, selected view)
  {
    const int tot = pool_total();
    pool_stat_g(4, tot);
    int q, r;
    for (int j = threadIdx.x; j < tot; j += blockDim.x) {
      pool_decode(j, q, r);
      const WeakPixel px = pix(q);
      const int ns = px.nsel();
      const int h = r / ns, k = r % ns;
      const int v = px.sel_list()[k] + 1;
      px.hv(2 + h)[k] = hyp_val_q(px, q, v, px.hyp()[h]);
    }
  }
  __syncthreads();
  PHASE(8);
  // ---- serial: sequential acceptance + write-back (DPE.cu:1190-1207, 1831-1843)
  if (active && c == 0) {
    if (has_fit) {
      for (int h = 0; h < 5; ++h) {
        const float4 tp = me.hyp()[h];
        const float tc = row_cost(2 + h);
        accept_if_better(tp, depth_from_plane(c0, tp, x, y), tc, dmin, dmax, depth_now, pnow, cost_now);
      }
    }
    float4 fin = cur;
    if (pc.P.state == DPE_REFINE_INIT) {
      if ((double)cost_now < (double)cost_written - 0.1) { fin = pnow; B.planes[center] = pnow; }
    } else {
      fin = pnow;
      B.planes[center] = pnow;
    }
    me.final_plane() = fin;
  }
  if (c == 0) me.pool_jobs() = active ? nsel : 0;
  __syncthreads();
  PHASE(9);
  // ---- phase 6: the stored cost is the Old NCC of the final plane (DPE.cu:1845-1861)
  {
    const int tot = pool_total();
    pool_stat_g(5, tot);
    int q, r;
    for (int j = threadIdx.x; j < tot; j += blockDim.x) {
      pool_decode(j, q, r);
      const WeakPixel px = pix(q);
      const int cq = list[wgbase + q];
      const int v = px.sel_list()[r] + 1;
      const float* os = px.osum();
      px.hv(0)[r] = ncc_old_any<U8>(fast_old, px.pw(), os[0], os[1], os[2], cq % W, cq / W, pc, B, v, px.final_plane());
    }
  }
  __syncthreads();
  PHASE(10);
  if (active && c == 0) B.costs[center] = row_cost(0);
  PHASE(11);
  PHASE_END(1);
}

}  // namespace dpe
