// viz.cpp — the reference's medium-result pictures on the host (ShowDepthMap / ShowNormalMap /
// ShowWeakImage, DPE.cpp:384-502) and the colours of EdgeSegment's img_connect.  The per-pixel
// rules are csrc/viz_render.h, which the device kernel shares.
#include "host.h"

#include "../csrc/viz_render.h"

namespace dpe_host {

void viz_render(int kind, int w, int h, const float* depth, const float* normal, const uint8_t* weak, float dmin,
                float dmax, uint8_t* bgr) {
  const size_t L = (size_t)w * h;
  for (size_t i = 0; i < L; ++i) {
    uint8_t* o = bgr + 3 * i;
    if (kind == DPE_VIZ_DEPTH) dpe_viz::depth_px(depth[i], dmin, dmax, o);
    else if (kind == DPE_VIZ_NORMAL) dpe_viz::normal_px(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], o);
    else dpe_viz::weak_px(weak[i], o);
  }
}

// colors[label] of img_connect (DPE.cpp:259-265).  The reference draws them from an unseeded,
// process-global rand(); here the colour is a fixed function of the label (a 32-bit integer hash),
// label 0 black.
void connect_color(int label, uint8_t* bgr) {
  bgr[0] = bgr[1] = bgr[2] = 0;
  if (label == 0) return;
  uint32_t x = (uint32_t)label;
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  bgr[0] = (uint8_t)x; bgr[1] = (uint8_t)(x >> 8); bgr[2] = (uint8_t)(x >> 16);
}

}  // namespace dpe_host

extern "C" int dpe_host_viz_render(int kind, int w, int h, const float* depth, const float* normal, const uint8_t* weak,
                                   float depth_min, float depth_max, uint8_t* bgr) {
  if (w < 1 || h < 1 || !bgr) return 1;
  if (kind == DPE_VIZ_DEPTH ? !depth : kind == DPE_VIZ_NORMAL ? !normal : kind == DPE_VIZ_WEAK ? !weak : true) return 1;
  dpe_host::viz_render(kind, w, h, depth, normal, weak, depth_min, depth_max, bgr);
  return 0;
}
