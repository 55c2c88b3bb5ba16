// dpe_edges.hip -- the EdgeSegment stages of include/dpe_mvs.h on the GPU (dpe_resize_linear,
// dpe_resize_u8, dpe_roberts_threshold, dpe_canny): the kernels of pass_edges.h over the context's
// edge scratch.  A unit of libdpe_mvs.so.  Each call uses the context's stream and synchronises it
// before it returns (the concurrency contract: dpe_mvs.hip).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "pass_edges.h"
#include "dpe_entry.h"
#include "dpe_context.h"

using namespace dpe;

namespace {
// cv::resize INTER_LINEAR CV_32F taps (host/hostio.cpp linear_taps)
void f32_taps(int n_src, int n_dst, int* s0, int* s1, float* a0, float* a1) {
  const double scale = 1.0 / ((double)n_dst / n_src);
  for (int d = 0; d < n_dst; ++d) {
    float f = (float)((d + 0.5) * scale - 0.5);
    int sidx = (int)std::floor(f);
    f -= (float)sidx;
    if (sidx < 0) { f = 0; sidx = 0; }
    if (sidx >= n_src - 1) { f = 0; sidx = n_src - 1; }
    s0[d] = sidx; s1[d] = std::min(sidx + 1, n_src - 1);
    a0[d] = 1.0f - f; a1[d] = f;
  }
}
// cv::resize INTER_LINEAR CV_8U taps (host/edges.cpp lin_tab): 11-bit weights, cvRound half to even
int u8_taps(int ssize, int dsize, int* ofs, short* a) {
  const double scale = 1.0 / ((double)dsize / ssize);
  int xmax = dsize;
  for (int d = 0; d < dsize; ++d) {
    float f = (float)((d + 0.5) * scale - 0.5);
    int sidx = (int)std::floor(f);
    f -= (float)sidx;
    if (sidx < 0) { f = 0; sidx = 0; }
    if (sidx + 1 >= ssize) {
      xmax = std::min(xmax, d);
      if (sidx >= ssize - 1) { f = 0; sidx = ssize - 1; }
    }
    ofs[d] = sidx;
    const float c0 = 1.0f - f, c1 = f;
    a[2 * d] = (short)std::min(32767, std::max(-32768, (int)std::nearbyint(c0 * 2048.0f)));
    a[2 * d + 1] = (short)std::min(32767, std::max(-32768, (int)std::nearbyint(c1 * 2048.0f)));
  }
  return xmax;
}
}  // namespace

extern "C" int dpe_resize_linear(DpeContext* c, const float* src, int w, int h, float* dst, int nw, int nh) {
  TRY(enter(c, src && dst && w >= 1 && h >= 1 && nw >= 1 && nh >= 1, "dpe_resize_linear: bad argument"));
  if (w == nw && h == nh) { std::memcpy(dst, src, sizeof(float) * (size_t)w * h); return DPE_OK; }
  EdgeScratch& e = c->edges;
  std::vector<int> it(2 * (size_t)(nw + nh));
  std::vector<float> ft(2 * (size_t)(nw + nh));
  f32_taps(w, nw, it.data(), it.data() + nw, ft.data(), ft.data() + nw);
  f32_taps(h, nh, it.data() + 2 * nw, it.data() + 2 * nw + nh, ft.data() + 2 * nw, ft.data() + 2 * nw + nh);
  HIPC(e.fa.ensure((size_t)w * h)); HIPC(e.fb.ensure((size_t)nw * nh));
  HIPC(e.rows.ensure((size_t)h * nw));   // f32 rows stored in the int scratch (same size)
  HIPC(e.itab.ensure(it.size())); HIPC(e.ftab.ensure(ft.size()));
  HIPC(hipMemcpyAsync(e.fa.p, src, sizeof(float) * (size_t)w * h, hipMemcpyHostToDevice, c->stream));
  HIPC(hipMemcpyAsync(e.itab.p, it.data(), it.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPC(hipMemcpyAsync(e.ftab.p, ft.data(), ft.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  float* rows = (float*)e.rows.p;
  const dim3 b(32, 8);
  k_resize_linear_h<<<dim3((nw + 31) / 32, (h + 7) / 8), b, 0, c->stream>>>(e.fa.p, w, h, e.itab.p, e.itab.p + nw,
                                                                            e.ftab.p, e.ftab.p + nw, rows, nw);
  k_resize_linear_v<<<dim3((nw + 31) / 32, (nh + 7) / 8), b, 0, c->stream>>>(rows, nw, e.itab.p + 2 * nw,
                                                                             e.itab.p + 2 * nw + nh, e.ftab.p + 2 * nw,
                                                                             e.ftab.p + 2 * nw + nh, e.fb.p, nh);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(dst, e.fb.p, sizeof(float) * (size_t)nw * nh, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  return DPE_OK;
}

// device-to-device core of dpe_resize_u8 (src / dst in the context's scratch)
static int resize_u8_dev(DpeContext* c, const uint8_t* dsrc, int w, int h, uint8_t* ddst, int nw, int nh) {
  const dim3 b(32, 8);
  if (w == nw && h == nh) { HIPC(hipMemcpyAsync(ddst, dsrc, (size_t)w * h, hipMemcpyDeviceToDevice, c->stream)); return DPE_OK; }
  const double scale_x = 1.0 / ((double)nw / w), scale_y = 1.0 / ((double)nh / h);
  const int isx = (int)std::lround(scale_x), isy = (int)std::lround(scale_y);
  const bool area_fast = std::fabs(scale_x - isx) < 2.220446049250313e-16 && std::fabs(scale_y - isy) < 2.220446049250313e-16;
  if (area_fast && isx == 2 && isy == 2) {   // INTER_LINEAR at exactly 1/2 = INTER_AREA's fast path
    k_resize_u8_half<<<dim3((nw + 31) / 32, (nh + 7) / 8), b, 0, c->stream>>>(dsrc, w, ddst, nw, nh);
    HIPC(hipGetLastError());
    return DPE_OK;
  }
  EdgeScratch& e = c->edges;
  std::vector<int> ofs((size_t)nw + nh);
  std::vector<short> a(2 * ((size_t)nw + nh));
  const int xmax = u8_taps(w, nw, ofs.data(), a.data());
  (void)u8_taps(h, nh, ofs.data() + nw, a.data() + 2 * nw);
  int xv = 0;                                 // VResizeLinear: 16-lane, then 8-lane vector blocks
  for (; xv <= nw - 16; xv += 16) {}
  for (; xv < nw - 8; xv += 8) {}
  HIPC(e.rows.ensure((size_t)h * nw)); HIPC(e.itab.ensure(ofs.size())); HIPC(e.stab.ensure(a.size()));
  HIPC(hipMemcpyAsync(e.itab.p, ofs.data(), ofs.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPC(hipMemcpyAsync(e.stab.p, a.data(), a.size() * sizeof(short), hipMemcpyHostToDevice, c->stream));
  k_resize_u8_h<<<dim3((nw + 31) / 32, (h + 7) / 8), b, 0, c->stream>>>(dsrc, w, h, e.itab.p, e.stab.p, xmax, e.rows.p, nw);
  k_resize_u8_v<<<dim3((nw + 31) / 32, (nh + 7) / 8), b, 0, c->stream>>>(e.rows.p, h, nw, e.itab.p + nw, e.stab.p + 2 * nw, xv,
                                                                         ddst, nh);
  HIPC(hipGetLastError());
  return DPE_OK;
}

extern "C" int dpe_resize_u8(DpeContext* c, const uint8_t* src, int w, int h, uint8_t* dst, int nw, int nh) {
  TRY(enter(c, src && dst && w >= 1 && h >= 1 && nw >= 1 && nh >= 1, "dpe_resize_u8: bad argument"));
  EdgeScratch& e = c->edges;
  HIPC(e.a.ensure((size_t)w * h)); HIPC(e.b.ensure((size_t)nw * nh));
  HIPC(hipMemcpyAsync(e.a.p, src, (size_t)w * h, hipMemcpyHostToDevice, c->stream));
  TRY(resize_u8_dev(c, e.a.p, w, h, e.b.p, nw, nh));
  HIPC(hipMemcpyAsync(dst, e.b.p, (size_t)nw * nh, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  return DPE_OK;
}

extern "C" int dpe_roberts_threshold(DpeContext* c, const uint8_t* src, int w, int h, int thr, uint8_t* dst) {
  TRY(enter(c, src && dst && w >= 1 && h >= 1, "dpe_roberts_threshold: bad argument"));
  EdgeScratch& e = c->edges;
  HIPC(e.a.ensure((size_t)w * h)); HIPC(e.b.ensure((size_t)w * h));
  HIPC(hipMemcpyAsync(e.a.p, src, (size_t)w * h, hipMemcpyHostToDevice, c->stream));
  k_roberts_threshold<<<dim3((w + 31) / 32, (h + 7) / 8), dim3(32, 8), 0, c->stream>>>(e.a.p, w, h, thr, e.b.p);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(dst, e.b.p, (size_t)w * h, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  return DPE_OK;
}

extern "C" int dpe_canny(DpeContext* c, const uint8_t* src, int w, int h, double low_thresh, double high_thresh, uint8_t* dst) {
  TRY(enter(c, src && dst && w >= 1 && h >= 1, "dpe_canny: bad argument"));
  Range range_("dpe_canny");
  if (low_thresh > high_thresh) std::swap(low_thresh, high_thresh);   // canny.cpp threshold handling
  low_thresh = std::min(32767.0, low_thresh);
  high_thresh = std::min(32767.0, high_thresh);
  if (low_thresh > 0) low_thresh *= low_thresh;
  if (high_thresh > 0) high_thresh *= high_thresh;
  const int low = (int)std::floor(low_thresh), high = (int)std::floor(high_thresh);
  const int ms = w + 2;
  const size_t L = (size_t)w * h, M = (size_t)ms * (h + 2);
  EdgeScratch& e = c->edges;
  HIPC(e.a.ensure(L)); HIPC(e.dx.ensure(L)); HIPC(e.dy.ensure(L)); HIPC(e.mag.ensure(M)); HIPC(e.map.ensure(M));
  HIPC(hipMemcpyAsync(e.a.p, src, L, hipMemcpyHostToDevice, c->stream));
  const dim3 b(32, 8), g((ms + 31) / 32, (h + 2 + 7) / 8);
  k_canny_sobel<<<g, b, 0, c->stream>>>(e.a.p, w, h, e.dx.p, e.dy.p, e.mag.p);
  k_canny_nms<<<g, b, 0, c->stream>>>(e.dx.p, e.dy.p, e.mag.p, w, h, low, high, e.map.p);
  HIPC(hipGetLastError());
  std::vector<uint8_t> map(M);
  HIPC(hipMemcpyAsync(map.data(), e.map.p, M, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  // hysteresis: 8-connected growth through candidates from every strong candidate (any order: the
  // closure is the same set)
  std::vector<size_t> stack;
  stack.reserve(L / 8 + 16);
  for (size_t i = 0; i < M; ++i) if (map[i] == 2) stack.push_back(i);
  const long off[8] = {-ms - 1, -ms, -ms + 1, -1, 1, ms - 1, ms, ms + 1};
  while (!stack.empty()) {
    const size_t i = stack.back();
    stack.pop_back();
    for (long o : off) {
      const size_t j = (size_t)((long)i + o);
      if (!map[j]) { map[j] = 2; stack.push_back(j); }
    }
  }
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) dst[(size_t)y * w + x] = map[(size_t)(y + 1) * ms + x + 1] == 2 ? 255 : 0;
  return DPE_OK;
}
