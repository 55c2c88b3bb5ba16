// pass_kernels.h — the kernels of one PatchMatch pass (DPE::RunPatchMatch, DPE.cu:3126-3249).
//
// Launch structure: full-grid kernels run one thread per pixel on 16x16 workgroups; the red/black
// sweeps run one thread per pixel of the colour on 32x4 workgroups (a wave covers two rows of 64
// columns).  Per-pixel arrays that the reference keeps in registers/local memory
// (cost_array[8][32], DPE.cu:1236/1690; p_costs[61], :2660) are staged in LDS, view-major with the
// thread index fastest, so every access is bank-conflict free.  The 36-tap Old-NCC reference patch
// (weights and weight*grey, view- and plane-independent) is computed once per pixel and kept in
// registers for every NCC the pixel evaluates in that launch.
#pragma once
#include "pass_common.h"

namespace dpe {

#define PIX2D_FULL()                                                   \
  const int lb_ = xcd_remap(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y, B.xcd_rows * gridDim.x); \
  const int x = (lb_ % gridDim.x) * blockDim.x + threadIdx.x;          \
  const int y = (lb_ / gridDim.x) * blockDim.y + threadIdx.y;          \
  if (x >= pc.W || y >= pc.H) return;                                  \
  const int center = x + y * pc.W;

// half-sweep pixel of colour `colour` (0 = black: (x+y) even, 1 = red), DPE.cu:1864-1938
#define PIX2D_HALF()                                                   \
  const int lb_ = xcd_remap(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y, B.xcd_rows * gridDim.x); \
  const int y = (lb_ / gridDim.x) * blockDim.y + threadIdx.y;          \
  const int x = 2 * ((lb_ % gridDim.x) * blockDim.x + threadIdx.x) + ((y + colour) & 1); \
  if (x >= pc.W || y >= pc.H || y >= pc.half_rows) return;             \
  const int center = x + y * pc.W;

// ------------------------------------------------------------------------------ GenEdgeInform
// The (2r+1)^2 window counts of the edge density come from a byte tile of the block's footprint in
// LDS (bit 0 edge, bit 1 label 0, bit 2 inside the image) for r <= kEiTileR; the counts are
// integers, so the tile changes nothing but the number of global loads (r^2 per pixel -> ~1.6).
constexpr int kEiTileR = 8, kEiTile = 16 + 2 * kEiTileR;
// GenEdgeInform's 8 edge rays (DPE.cu:2497-2530: the first edge pixel along each direction, to the
// image border) as line scans: every pixel lies on one row, one column, one diagonal (x - y const)
// and one anti-diagonal (x + y const); along a line the ray in one direction is the nearest edge
// position after the pixel, in the other the nearest before it.  One wave per line, 64 consecutive
// positions per step: the edge bits of a step by ballot, the nearest set bit above / below each lane
// by bit arithmetic, the nearest edge beyond the step carried from the steps already done (the
// lines are walked once from each end).  Same positions as the per-pixel walks, O(L) loads in all.
__global__ void __launch_bounds__(64) k_edge_rays(const PassConst* __restrict__ pcp, DevBufs B) {
  const PassConst& pc = *pcp;
  const int W = pc.W, H = pc.H;
  const int lane = threadIdx.x;
  int line = blockIdx.x;
  // family f: 0 rows (kDir 2 / 3), 1 columns (0 / 1), 2 diagonals (4 / 5), 3 anti-diagonals (7 / 6);
  // position t along the line, pixel (x0 + t * sx, y0 + t * sy), t in [0, len)
  int f, x0, y0, sx, sy, len, iprev, inext;
  if (line < H) { f = 0; x0 = 0; y0 = line; sx = 1; sy = 0; len = W; iprev = 2; inext = 3; }
  else if ((line -= H) < W) { f = 1; x0 = line; y0 = 0; sx = 0; sy = 1; len = H; iprev = 0; inext = 1; }
  else if ((line -= W) < W + H - 1) {   // x - y = c, c = line - (H - 1), t = y - max(0, -c)
    f = 2; const int c = line - (H - 1);
    y0 = c < 0 ? -c : 0; x0 = c + y0; sx = 1; sy = 1; len = MINo(H - y0, W - x0); iprev = 4; inext = 5;
  } else {                              // x + y = s, t = y - max(0, s - W + 1)
    line -= W + H - 1; f = 3; const int sm = line;
    y0 = sm - (W - 1) > 0 ? sm - (W - 1) : 0; x0 = sm - y0; sx = -1; sy = 1; len = MINo(H - y0, x0 + 1); iprev = 7; inext = 6;
  }
  (void)f;
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  const unsigned long long above = lane == 63 ? 0ull : (~0ull << (lane + 1));
  // forward: nearest edge before t (direction iprev)
  int carry = -1;
  for (int t0 = 0; t0 < len; t0 += 64) {
    const int t = t0 + lane;
    const int px = x0 + t * sx, py = y0 + t * sy;
    const bool e = t < len && B.edge[py * W + px] != 0;
    const unsigned long long m = __ballot(e);
    const unsigned long long lo = m & below;
    const int prev = lo ? t0 + 63 - __builtin_clzll(lo) : carry;
    if (t < len) {
      B.edge_neigh[(size_t)(py * W + px) * 8 + iprev] =
          prev < 0 ? make_short2(-1, -1) : make_short2((short)(x0 + prev * sx), (short)(y0 + prev * sy));
    }
    if (m) carry = t0 + 63 - __builtin_clzll(m);
  }
  // backward: nearest edge after t (direction inext)
  carry = -1;
  for (int t0 = ((len - 1) / 64) * 64; t0 >= 0; t0 -= 64) {
    const int t = t0 + lane;
    const int px = x0 + t * sx, py = y0 + t * sy;
    const bool e = t < len && B.edge[py * W + px] != 0;
    const unsigned long long m = __ballot(e);
    const unsigned long long hi = m & above;
    const int next = hi ? t0 + __builtin_ctzll(hi) : carry;
    if (t < len) {
      B.edge_neigh[(size_t)(py * W + px) * 8 + inext] =
          next < 0 ? make_short2(-1, -1) : make_short2((short)(x0 + next * sx), (short)(y0 + next * sy));
    }
    if (m) carry = t0 + __builtin_ctzll(m);
  }
}

__global__ void __launch_bounds__(256) k_gen_edge_inform(const PassConst* __restrict__ pcp, DevBufs B) {   // DPE.cu:2483-2591
  const PassConst& pc = *pcp;
  __shared__ uint8_t s_tile[kEiTile * kEiTile];
  __shared__ uint32_t s_hs[kEiTile][16];   // round 6: row sums of the packed flags over 2r + 1 columns
  const int radius = pc.P.strong_radius;
  const bool tiled = pc.P.use_edge && radius >= 0 && radius <= kEiTileR && blockDim.x == 16;
  if (tiled) {   // block-uniform; every thread of the block helps before any returns
    const int lb0 = xcd_remap(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y, B.xcd_rows * gridDim.x);
    const int ox = (lb0 % gridDim.x) * blockDim.x - radius, oy = (lb0 / gridDim.x) * blockDim.y - radius;
    const int tw = blockDim.x + 2 * radius, th = blockDim.y + 2 * radius;
    for (int t = threadIdx.y * blockDim.x + threadIdx.x; t < tw * th; t += blockDim.x * blockDim.y) {
      const int nx = ox + t % tw, ny = oy + t / tw;
      uint8_t v = 0;
      if (nx >= 0 && nx < pc.W && ny >= 0 && ny < pc.H) {
        const int q = ny * pc.W + nx;
        v = 4 | (B.edge[q] ? 1 : 0) | ((pc.P.use_label && B.label[q] == 0) ? 2 : 0);
      }
      s_tile[t] = v;
    }
    __syncthreads();
    // the window counts are separable: each (tile row, output column) sums its 2r + 1 flags, packed
    // as edge | label 0 << 10 | inside << 20 (each count <= 17 x 17 < 1024), then a pixel adds 2r + 1
    // row sums -- the same integer counts as the 2-D loop
    for (int t = threadIdx.y * blockDim.x + threadIdx.x; t < th * 16; t += blockDim.x * blockDim.y) {
      const uint8_t* row = s_tile + (t / 16) * tw + t % 16;
      uint32_t acc = 0;
      for (int i = 0; i <= 2 * radius; i++) {
        const uint32_t v = row[i];
        acc += (v & 1u) | ((v & 2u) << 9) | ((v & 4u) << 18);
      }
      s_hs[t / 16][t % 16] = acc;
    }
    __syncthreads();
  }
  PIX2D_FULL();
  const int W = pc.W, H = pc.H;
  if (pc.P.use_edge) {   // the 8 edge rays come from k_edge_rays
    int edge_pix = 0, tot_pix = 0, bound_pix = 0;
    if (tiled) {
      uint32_t acc = 0;
      for (int j = 0; j <= 2 * radius; j++) acc += s_hs[threadIdx.y + j][threadIdx.x];
      edge_pix = (int)(acc & 1023u); bound_pix = (int)((acc >> 10) & 1023u); tot_pix = (int)(acc >> 20);
    } else {
      for (int i = -radius; i <= radius; i++)
        for (int j = -radius; j <= radius; j++) {
          const int nx = x + i, ny = y + j;
          if (nx < 0 || nx >= W || ny < 0 || ny >= H) continue;
          if (B.edge[ny * W + nx]) edge_pix++;
          if (pc.P.use_label && B.label[ny * W + nx] == 0) bound_pix++;
          tot_pix++;
        }
    }
    float density = 1.0f * edge_pix / tot_pix;
    if (pc.P.use_label) density = MAXo(density, (float)(bound_pix / tot_pix));   // integer division (:2551)
    B.complex_[center] = (float)(1.0f / (1.0f + d_exp_d(-25.0 * ((double)density - 0.35))));
  }
  if (pc.P.use_label && B.weak[center] == DPE_WEAK) {
    const int cl = B.label[center];
    if (cl > 0) {
      short2* lb = B.lab_bound + (size_t)center * 8;
      for (int i = 0; i < 8; i++) {
        // last pixel of the own label before the first -1 label (or the border); batches of 8 loads
        const int dx = kDir[i][0], dy = kDir[i][1];
        const int sx = dx > 0 ? W - 1 - x : (dx < 0 ? x : 1 << 30);
        const int sy = dy > 0 ? H - 1 - y : (dy < 0 ? y : 1 << 30);
        const int n = MINo(sx, sy);
        int lk = -1;
        bool stop = false;
        for (int k0 = 1; k0 <= n && !stop; k0 += 8) {
          int lab[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) lab[k] = (k0 + k <= n) ? B.label[(x + (k0 + k) * dx) + (y + (k0 + k) * dy) * W] : -1;
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            if (stop) continue;
            if (k0 + k > n) { stop = true; continue; }
            if (lab[k] == cl) lk = k0 + k;
            else if (lab[k] == -1) stop = true;
          }
        }
        lb[i] = lk < 0 ? make_short2(-1, -1) : make_short2((short)(x + lk * dx), (short)(y + lk * dy));
      }
    }
  }
}

// ------------------------------------------------------------------------------ RandomInitialization
template <int U8>
__global__ void __launch_bounds__(256) k_random_init(const PassConst* __restrict__ pcp, DevBufs B) {   // DPE.cu:1035-1063
  const PassConst& pc = *pcp;
  PIX2D_FULL();
  const DpeCamera& c0 = pc.cams[0];
  const int N = pc.N;
  const bool fast = FAST_PATCH(pc);
  Patch36 P;
  if (fast) make_patch36(P, pc, B, x, y); else { P.px = x; P.py = y; }
  if (pc.P.state == DPE_FIRST_INIT) {
    Rng rs; rng_init(rs, (uint32_t)center, pc.seed32, STREAM_RANDOM_INIT, pc.salt);
    const float depth = rng_uniform(rs) * (pc.P.depth_max - pc.P.depth_min) + pc.P.depth_min;
    float4 ph = random_normal(c0, x, y, rs, depth);
    ph.w = dist2origin(c0, x, y, depth, ph);
    B.planes[center] = ph;
    // ComputeMultiViewInitialCostandSelectedViews (DPE.cu:780-826): sorted copy kept in registers
    float sorted[DPE_MAX_IMAGES];
    int cost_count = 0, num_valid = 0;
    for (int i = 1; i < N; ++i) {
      const float c = ncc_old<U8>(P, fast, pc, B, i, ph);
      // insertion into the sorted prefix == sort_small of the full vector afterwards
      int j = cost_count;
      for (; j >= 1 && c < sorted[j - 1]; j--) sorted[j] = sorted[j - 1];
      sorted[j] = c;
      cost_count++;
      if (c < 2.0f) num_valid++;
    }
    uint32_t sel = 0;
    const int top_k = MINo(num_valid, pc.P.top_k);
    float cost = 2.0f;
    if (top_k > 0) {
      float s = 0.0f;
      for (int i = 0; i < top_k; ++i) s += sorted[i];
      const float thr = sorted[top_k - 1];
      // second pass recomputes the (deterministic) per-view costs instead of keeping a copy
      for (int i = 1; i < N; ++i) if (ncc_old<U8>(P, fast, pc, B, i, ph) <= thr) setBit(sel, i - 1);
      cost = s / top_k;
    }
    B.sel[center] = sel;
    B.costs[center] = cost;
  } else {
    float4 ph = transform_normal_ref(c0, B.planes[center]);
    const float depth = ph.w;
    ph.w = dist2origin(c0, x, y, depth, ph);
    B.planes[center] = ph;
    // ComputeMultiViewInitialCost (DPE.cu:828-857)
    uint32_t sel = B.sel[center];
    int cc = 0; float cost = 0.0f;
    for (int i = 1; i < N; ++i) {
      if (isSet(sel, i - 1)) {
        const float c = ncc_old<U8>(P, fast, pc, B, i, ph);
        if (c < 2.0f) { cc++; cost += c; }
        else unSetBit(sel, i - 1);
      }
    }
    B.sel[center] = sel;
    B.costs[center] = cc == 0 ? 2.0f : cost / cc;
  }
}

// ------------------------------------------------------------------------------ GetDepthandNormal
__global__ void k_depth_normal(const PassConst* __restrict__ pcp, DevBufs B) {   // DPE.cu:1940-1955
  const PassConst& pc = *pcp;
  PIX2D_FULL();
  float4 p = B.planes[center];
  p.w = depth_from_plane(pc.cams[0], p, x, y);
  B.planes[center] = transform_normal(pc.cams[0], p);
}

// ------------------------------------------------------------------------------ CheckerboardFilterStrong
// The up-to-21 candidates live in LDS, thread index fastest (conflict-free), so the insertion sort
// indexes them without scratch memory.  Launched with 128-thread (32 x 4) workgroups.
constexpr int kFilterThreads = 128;
__global__ void __launch_bounds__(kFilterThreads) k_filter(const PassConst* __restrict__ pcp, DevBufs B, int colour) {   // DPE.cu:1957-2101
  __shared__ float s_filter[21][kFilterThreads];
  const PassConst& pc = *pcp;
  PIX2D_HALF();
  const int W = pc.W, H = pc.H;
  if (B.weak[center] == DPE_WEAK) return;
  const float4* P = B.planes;
  struct Col {
    float* p;
    DEV float& operator[](int i) const { return p[i * kFilterThreads]; }
  } filter{&s_filter[0][threadIdx.y * blockDim.x + threadIdx.x]};
  int n = 0;
  filter[n++] = P[center].w;
  if (B.costs[center] < 0.001f) return;
  const int left = center - 1, leftleft = center - 3, up = center - W, upup = center - 3 * W;
  const int down = center + W, downdown = center + 3 * W, right = center + 1, rightright = center + 3;
  auto add = [&](bool cond, int idx) { if (cond && B.weak[idx] == DPE_STRONG) filter[n++] = P[idx].w; };
  add(y > 0, up); add(y > 2, upup); add(y > 4, upup - W * 2);
  add(y < H - 1, down); add(y < H - 3, downdown); add(y < H - 5, downdown + W * 2);
  add(x > 0, left); add(x > 2, leftleft); add(x > 4, leftleft - 2);
  add(x < W - 1, right); add(x < W - 3, rightright); add(x < W - 5, rightright + 2);
  add(y > 0 && x < W - 2, up + 2); add(y < H - 1 && x < W - 2, down + 2);
  add(y > 0 && x > 1, up - 2); add(y < H - 1 && x > 1, down - 2);
  add(x > 0 && y > 2, left - W * 2); add(x < W - 1 && y > 2, right - W * 2);
  add(x > 0 && y < H - 2, left + W * 2); add(x < W - 1 && y < H - 2, right + W * 2);
  for (int i = 1; i < n; i++) {
    const float tmp = filter[i];
    int j = i;
    for (; j >= 1 && tmp < filter[j - 1]; j--) filter[j] = filter[j - 1];
    filter[j] = tmp;
  }
  const int m = n / 2;
  B.planes[center].w = (n % 2 == 0) ? (filter[m - 1] + filter[m]) / 2 : filter[m];
}

// ------------------------------------------------------------------------------ staging kernels
// padded quad-texel images of 8-bit (or quarter-integer: q8 == nullptr) grey levels, both layouts
// (pass_common.h: TEX_U8, TEX_F16)
__global__ void k_build_quad8(const float* __restrict__ img, uint32_t* __restrict__ q8, uint2* __restrict__ q16,
                              int W, int H) {
  const int X = blockIdx.x * blockDim.x + threadIdx.x;
  const int Y = blockIdx.y * blockDim.y + threadIdx.y;
  if (X > W + 1 || Y > H + 1) return;
  auto cl = [](int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); };
  const int x0 = cl(X - 1, W), x1 = cl(X, W), y0 = cl(Y - 1, H), y1 = cl(Y, H);
  const float a = img[y0 * W + x0], b = img[y0 * W + x1], c = img[y1 * W + x0], d = img[y1 * W + x1];
  const size_t o = (size_t)Y * (W + 2) + X;
  if (q8) q8[o] = (uint32_t)a | ((uint32_t)b << 8) | ((uint32_t)c << 16) | ((uint32_t)d << 24);
  const h2v lo = (h2v){(_Float16)a, (_Float16)c};
  const h2v df = (h2v){(_Float16)(b - a), (_Float16)(d - c)};
  q16[o] = make_uint2(__builtin_bit_cast(uint32_t, lo), __builtin_bit_cast(uint32_t, df));
}
// TEX_P16 column pairs (pass_common.h): (g(X-1, Y-1), g(X-1, Y)) as f16, X in [0, W+2], Y in [0, H+1]
__global__ void k_build_pair16(const float* __restrict__ img, uint32_t* __restrict__ qp, int W, int H) {
  const int X = blockIdx.x * blockDim.x + threadIdx.x;
  const int Y = blockIdx.y * blockDim.y + threadIdx.y;
  if (X > W + 2 || Y > H + 1) return;
  auto cl = [](int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); };
  const int x0 = cl(X - 1, W), y0 = cl(Y - 1, H), y1 = cl(Y, H);
  const h2v pr = (h2v){(_Float16)img[y0 * W + x0], (_Float16)img[y1 * W + x0]};
  qp[(size_t)Y * (W + 3) + X] = __builtin_bit_cast(uint32_t, pr);
}
// padded quad-texel image (see pass_common.h)
__global__ void k_build_quad(const float* __restrict__ img, float4* __restrict__ q, int W, int H) {
  const int X = blockIdx.x * blockDim.x + threadIdx.x;
  const int Y = blockIdx.y * blockDim.y + threadIdx.y;
  if (X > W + 1 || Y > H + 1) return;
  auto cl = [](int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); };
  const int x0 = cl(X - 1, W), x1 = cl(X, W), y0 = cl(Y - 1, H), y1 = cl(Y, H);
  q[Y * (W + 2) + X] = make_float4(img[y0 * W + x0], img[y0 * W + x1], img[y1 * W + x0], img[y1 * W + x1]);
}

}  // namespace dpe
