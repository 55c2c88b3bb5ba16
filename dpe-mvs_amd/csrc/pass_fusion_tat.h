// pass_fusion_tat.h — the two Tanks-and-Temples fusions, RunFusion_TAT_Intermediate (DPE.cpp:1372-1540)
// and RunFusion_TAT_advanced (DPE.cpp:1542-1689), one whole image on the GPU.
//
// Unlike RunFusion these variants set only the fused pixel's OWN mask and read the masks of the source
// views, which are other images: final when that image was fused earlier, all zero when it comes
// later.  So the pixels of one image are independent and only the images are sequential -- with one
// exception the reference carries as a defect: its per-view `diff` entries are declared outside the
// pixel loops (DPE.cpp:1462, :1626) and never reset, so a view that does not hit at a pixel keeps the
// entry of the last pixel, in raster order, where it did.  That is a last-valid carry:
//
//   k_tat_hit_scan     per pixel p and view j: q = p when p is active and hits view j, else -1, and
//                      the inclusive max-scan of q over the 256 pixels of the block (last[j][p]); the
//                      block's maximum goes to agg[j][chunk]
//   k_tat_chunk_carry  per view: exclusive max-scan of agg over the chunks, in place; with it the
//                      carry crosses row ends and chunk ends
//   k_tat_decide       per active pixel: the entry of view j is recomputed at q = max(last, carry)
//                      (only the 4-byte index is stored, not the 20-byte entry: most pixels hit
//                      themselves, and the entry is a pure function of q and j); the k loop, the
//                      colour, the pixel's own mask, the point into rec[p], emit[p], and the block's
//                      point count into cnt[chunk]
//   k_offsets_scan     (block_scan.h) exclusive sum-scan of cnt over the chunks, the total into *tot
//   k_tat_fill         stable compaction of rec into out (image raster order)
//
// Arithmetic as in pass_fusion.h: the reference's expression order in single precision
// (-ffp-contract=off), the reprojection error in double rounded once.  The angle test
// `GetAngle(n_ref, n_src) < T_k` needs no device acosf: the entry carries the dot product and the host
// passes D[k], the smallest float in [-1, 1] whose acosf is below T_k (host/fusion_tat.cpp), so the
// test is fz_angle_ok(dot, D[k]) (fusion_world.h).
#pragma once
#include "block_scan.h"
#include "pass_fusion.h"

namespace dpe {

constexpr int kTatChunk = 256;     // pixels per block of the scan, decide and fill kernels
constexpr int kTatMaxSrc = 31;     // source views per image: one bit per k in the decide kernel

// (TatViewDev and TatPoint: dpe_fusion_types.h)
struct TatEntry { float dist, depth, dot; int sp; };

// DPE.cpp:1465-1471: the pixels the walk does not skip
__device__ inline bool tat_active(const FusionViewDev& R, const uint8_t* block, int p, float& ref_depth) {
  if (block && block[p] < 128) return false;
  ref_depth = R.depth[p];
  if (ref_depth <= 0.0f) return false;
  return true;
}

// DPE.cpp:1481-1489: source pixel of the projection when it lies inside the view, is not masked and
// has a depth; else -1.  The in-range test on the float (fz_pixel).
__device__ inline int tat_hit(const FP3& X, const FusionViewDev& S, const DpeCamera& sc, const uint8_t* smask) {
  int src_c, src_r;
  if (!fz_pixel(X, sc, S.w, S.h, src_c, src_r)) return -1;
  const int sp = src_r * S.w + src_c;
  if (smask[sp] == 1) return -1;
  if (S.depth[sp] <= 0.0f) return -1;
  return sp;
}

// DPE.cpp:1490-1501: the entry pixel q of the reference view writes for a view it hits at sp
__device__ inline TatEntry tat_entry(const FusionViewDev& R, const DpeCamera& rc, int q, const FusionViewDev& S,
                                     const DpeCamera& sc, int sp) {
  const int r = q / R.w, c = q - r * R.w;
  const int src_r = sp / S.w, src_c = sp - src_r * S.w;
  const FzPair d = fz_pair(c, r, R.depth[q], rc, src_c, src_r, S.depth[sp], sc);
  TatEntry e;
  e.dist = d.dist;
  e.depth = d.depth;
  e.dot = fz_dot(R.normal + 3 * (size_t)q, S.normal + 3 * (size_t)sp);
  e.sp = sp;
  return e;
}

// last[j*L + p]: the largest pixel q <= p of p's block that is active and hits view src[j], else -1;
// agg[j*nch + block]: the same over the whole block.
__global__ void __launch_bounds__(kTatChunk) k_tat_hit_scan(const DpeCamera* __restrict__ cams,
                                                            const FusionViewDev* __restrict__ views,
                                                            const TatViewDev* __restrict__ tviews, int ref,
                                                            const int* __restrict__ src, int ns, int nch,
                                                            int* __restrict__ last, int* __restrict__ agg) {
  __shared__ int s4[4];
  const FusionViewDev R = views[ref];
  const int L = R.w * R.h;
  const int p = blockIdx.x * kTatChunk + threadIdx.x;
  float ref_depth = 0.0f;
  const bool act = p < L && tat_active(R, tviews[ref].block, p, ref_depth);
  FP3 X{0.0f, 0.0f, 0.0f};
  if (act) {
    const int r = p / R.w, c = p - r * R.w;
    X = fz_world(c, r, ref_depth, cams[ref]);
  }
  for (int j = 0; j < ns; ++j) {
    const int s = src[j];
    const int v = act && tat_hit(X, views[s], cams[s], tviews[s].mask) >= 0 ? p : -1;
    int all;
    const int incl = block_scan<ScanMax>(v, s4, &all);
    if (p < L) last[(size_t)j * L + p] = incl;
    if (threadIdx.x == 0) agg[j * nch + blockIdx.x] = all;
  }
}

// per view (one block each): agg[j*nch + k] becomes the maximum over the chunks before k, or -1
__global__ void __launch_bounds__(256) k_tat_chunk_carry(int nch, int* __restrict__ agg) {
  __shared__ int s4[4];
  __shared__ int sh[256];
  int* a = agg + (size_t)blockIdx.x * nch;
  int acc = -1;   // the maximum over the tiles before this one
  for (int k0 = 0; k0 < nch; k0 += 256) {
    const int k = k0 + (int)threadIdx.x;
    int all;
    sh[threadIdx.x] = block_scan<ScanMax>(k < nch ? a[k] : -1, s4, &all);
    __syncthreads();
    const int before = threadIdx.x > 0 ? sh[threadIdx.x - 1] : -1;
    __syncthreads();
    if (k < nch) a[k] = max(acc, before);
    acc = max(acc, all);
  }
}

// The entry view src[j] carries at pixel p of chunk blockIdx.x: recomputed at q = max(last, carry), the last pixel
// up to p that is active and hits the view.  False when there is none so far (the reference's entry is then FLT_MAX
// in all three tests); else sv = src[j] and the entry.
__device__ inline bool tat_carried(int j, int p, int L, int nch, const int* __restrict__ last, const int* __restrict__ agg,
                                   const FusionViewDev& R, const DpeCamera& rc, const DpeCamera* __restrict__ cams,
                                   const FusionViewDev* __restrict__ views, const TatViewDev* __restrict__ tviews,
                                   const int* __restrict__ src, int& sv, TatEntry& e) {
  const int q = max(last[(size_t)j * L + p], agg[j * nch + blockIdx.x]);
  if (q < 0) return false;
  sv = src[j];
  const FusionViewDev S = views[sv];
  const DpeCamera& sc = cams[sv];
  const int qr = q / R.w, qc = q - qr * R.w;
  const int sp = tat_hit(fz_world(qc, qr, R.depth[q], rc), S, sc, tviews[sv].mask);   // the hit k_tat_hit_scan found
  if (sp < 0) return false;
  e = tat_entry(R, rc, q, S, sc, sp);
  return true;
}

// The k loop of one pixel (DPE.cpp:1504-1534 / :1668-1683).  mode 1 = Intermediate, 2 = Advanced.
// dthr[k]: the dot-product threshold of the angle test at k (Intermediate).
__global__ void __launch_bounds__(kTatChunk) k_tat_decide(const DpeCamera* __restrict__ cams,
                                                          const FusionViewDev* __restrict__ views,
                                                          const TatViewDev* __restrict__ tviews, int ref,
                                                          const int* __restrict__ src, int ns, int nch, int mode,
                                                          const float* __restrict__ dthr, const int* __restrict__ last,
                                                          const int* __restrict__ agg, TatPoint* __restrict__ rec,
                                                          uint8_t* __restrict__ emit, int* __restrict__ cnt) {
  __shared__ int s4[4];
  const FusionViewDev R = views[ref];
  const TatViewDev TR = tviews[ref];
  const DpeCamera& rc = cams[ref];
  const int L = R.w * R.h;
  const int p = blockIdx.x * kTatChunk + threadIdx.x;
  const float dist_base = 0.25f;
  const float depth_base = mode == 1 ? 1.0f / 3500.0f : 1.0f / 3000.0f;
  float ref_depth = 0.0f;
  const bool act = p < L && tat_active(R, TR.block, p, ref_depth);
  int kept = 0;          // the k at which the pixel is fused, 0: not fused
  int count = 0;
  if (act) {
    // bit k of use_j: view j passes the tests at k.  The per-k counts are kept as vertical counters:
    // bit k of plane[b] is bit b of count(k).
    uint32_t plane[5] = {0u, 0u, 0u, 0u, 0u};
    for (int j = 0; j < ns; ++j) {
      int sv;
      TatEntry e;
      if (!tat_carried(j, p, L, nch, last, agg, R, rc, cams, views, tviews, src, sv, e)) continue;
      uint32_t use = 0u;
      for (int k = 2; k <= ns; ++k) {
        bool u = e.dist < k * dist_base && e.depth < k * depth_base;
        if (mode == 1) u = u && fz_angle_ok(e.dot, dthr[k]);
        use |= (uint32_t)u << k;
      }
      uint32_t carry = use;
#pragma unroll
      for (int b = 0; b < 5; ++b) {
        const uint32_t t = plane[b] & carry;
        plane[b] ^= carry;
        carry = t;
      }
    }
    for (int k = 2; k <= ns && !kept; ++k) {
      int n = 0;
#pragma unroll
      for (int b = 0; b < 5; ++b) n |= (int)((plane[b] >> k) & 1u) << b;
      if (n >= k) { kept = k; count = n; }
    }
  }
  if (kept) {
    const int r = p / R.w, c = p - r * R.w;
    float col[3] = {(float)TR.bgr[3 * (size_t)p], (float)TR.bgr[3 * (size_t)p + 1], (float)TR.bgr[3 * (size_t)p + 2]};
    if (mode == 1) {   // the colours of the views used at `kept`, ascending j (DPE.cpp:1515-1526)
      for (int j = 0; j < ns; ++j) {
        int sv;
        TatEntry e;
        if (!tat_carried(j, p, L, nch, last, agg, R, rc, cams, views, tviews, src, sv, e)) continue;
        if (e.dist < kept * dist_base && e.depth < kept * depth_base && fz_angle_ok(e.dot, dthr[kept])) {
          const uint8_t* sb = tviews[sv].bgr + 3 * (size_t)e.sp;
          col[0] += (float)sb[0];
          col[1] += (float)sb[1];
          col[2] += (float)sb[2];
        }
      }
      col[0] /= (count + 1.0f);
      col[1] /= (count + 1.0f);
      col[2] /= (count + 1.0f);
    }
    const FP3 X = fz_world(c, r, ref_depth, rc);
    rec[p] = TatPoint{X.x, X.y, X.z, col[0], col[1], col[2]};
    TR.mask[p] = 1;
  }
  if (p < L) emit[p] = kept ? 1 : 0;
  int n = kept ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = s4[0] + s4[1] + s4[2] + s4[3];
}

// out[off[chunk] + rank of p among the chunk's fused pixels] = rec[p]: raster order
__global__ void __launch_bounds__(kTatChunk) k_tat_fill(int L, const uint8_t* __restrict__ emit,
                                                        const TatPoint* __restrict__ rec, const int* __restrict__ off,
                                                        TatPoint* __restrict__ out) {
  __shared__ int s4[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = blockIdx.x * kTatChunk + threadIdx.x;
  const bool e = p < L && emit[p] != 0;
  const unsigned long long m = __ballot(e);
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  if (lane == 0) s4[wave] = __popcll(m);
  __syncthreads();
  int a = off[blockIdx.x] + __popcll(m & below);
  for (int w = 0; w < wave; ++w) a += s4[w];
  if (e) out[a] = rec[p];
}

}  // namespace dpe
