// pass_viz.h — the viz medium results on the device (dpe_state_render*, include/dpe_mvs.h): the
// reference's ShowDepthMap / ShowNormalMap / ShowWeakImage pictures from an HBM-resident state and
// the data-parallel half of the JPEG encode that cv::imwrite would run on them.  The per-pixel
// rules (viz_render.h) and the encoder arithmetic (jpeg_front.h) are the functions the host
// restatements call, so the results are bit-identical to dpe_host_viz_render / dpe_host_jpeg_blocks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpeg_front.h"
#include "viz_render.h"

namespace dpe {

// One thread per 4 pixels (12 output bytes, three aligned 32-bit stores; the tail by bytes).
// planes = (world normal xyz, depth) after the epilogue, weak = PixelState; bgr holds 3 * L bytes.
__global__ __launch_bounds__(256) void k_viz_render(int kind, const float4* __restrict__ planes,
                                                    const uint8_t* __restrict__ weak, float dmin, float dmax,
                                                    uint8_t* __restrict__ bgr, size_t L) {
  const size_t i0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i0 >= L) return;
  uint32_t b[12];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint8_t o[3] = {0, 0, 0};
    const size_t i = i0 + k;
    if (i < L) {
      if (kind == dpe_viz::KIND_DEPTH) dpe_viz::depth_px(planes[i].w, dmin, dmax, o);
      else if (kind == dpe_viz::KIND_NORMAL) { const float4 p = planes[i]; dpe_viz::normal_px(p.x, p.y, p.z, o); }
      else dpe_viz::weak_px(weak[i], o);
    }
    b[3 * k] = o[0]; b[3 * k + 1] = o[1]; b[3 * k + 2] = o[2];
  }
  if (i0 + 4 <= L) {
    uint32_t* out = reinterpret_cast<uint32_t*>(bgr + 3 * i0);   // 12 * thread bytes from a 256-byte aligned base
    out[0] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    out[1] = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
    out[2] = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (i0 + k / 3 < L) bgr[3 * i0 + k] = (uint8_t)b[k];
  }
}

__device__ __forceinline__ int viz_pick8(const int* d, int i) {
  int v = d[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) v = i == k ? d[k] : v;
  return v;
}

// JPEG front half of an 8-bit BGR image (4:2:0): one workgroup per 16x16 MCU, one 64-lane wave per
// 8x8 block (Y00 Y01 Y10 Y11 Cb Cr), one lane per sample.  Samples (colour conversion, chroma
// averaging, edge replication by clamped reads, level shift) go to LDS; every lane then runs the
// 1-D DCT of its row and keeps its column's output, the same again for the columns, and
// quantises with the tables in LDS.  qtab = 64 luma + 64 chroma entries, natural order; blocks
// receives gridDim.x * gridDim.y * 6 * 64 int16 in scan order.  The eight-fold redundant 1-D DCT
// keeps every lane busy and needs no cross-lane traffic beyond the two tile exchanges; the pick
// of one of its eight outputs is a lane-dependent index, which the compiler serves from LDS
// (14 KB per workgroup in all, no scratch: `make resource-usage`).
__global__ __launch_bounds__(384) void k_jpeg_front(const uint8_t* __restrict__ bgr, int w, int h,
                                                    const uint16_t* __restrict__ qtab, int16_t* __restrict__ blocks) {
  __shared__ int tile[6][64];
  __shared__ uint16_t q[128];
  const int t = threadIdx.x, k = t >> 6, lane = t & 63, r = lane >> 3, c = lane & 7;
  if (t < 128) q[t] = qtab[t];
  const int mx = blockIdx.x, my = blockIdx.y;
  int comp, bx, by;
  bool dummy;
  dpe_jpeg::block_source(w, h, 3, mx, my, k, &comp, &bx, &by, &dummy);
  tile[k][lane] = dpe_jpeg::sample(bgr, w, h, 3, comp, bx * 8 + c, by * 8 + r);
  __syncthreads();
  int d[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) d[i] = tile[k][r * 8 + i];
  dpe_jpeg::fdct_1d(d, 1);
  int v = viz_pick8(d, c);
  __syncthreads();
  tile[k][lane] = v;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i) d[i] = tile[k][i * 8 + c];
  dpe_jpeg::fdct_1d(d, 2);
  v = dpe_jpeg::quantise(viz_pick8(d, r), q[(comp ? 64 : 0) + lane]);
  if (dummy && lane) v = 0;
  blocks[(((size_t)my * gridDim.x + mx) * 6 + k) * 64 + lane] = (int16_t)v;
}

}  // namespace dpe
