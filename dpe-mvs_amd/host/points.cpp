// points.cpp — ExportDepthImagePointCloud (DPE.cpp:1691-1724) and the RescaleImageAndCamera
// (DPE.cpp:1123-1144) it shares with the fusions, on the host: the yardstick of the device path
// (csrc/pass_points.h) and what DpePipelineOptions.point_cloud runs with a runner hook (no GPU).
#include "host.h"

#include <cstring>

namespace dpe_host {

// the intrinsics of an image resized by (sx, sy) (DPE.cpp:812-815, 1139-1142)
void scale_intrinsics(DpeCamera& cam, float sx, float sy) { cam.K[0] *= sx; cam.K[2] *= sx; cam.K[4] *= sy; cam.K[5] *= sy; }

void resize_bgr_and_camera(const ColorImage& img, int w, int h, DpeCamera& cam, std::vector<uint8_t>& bgr) {
  std::vector<uint8_t> ch((size_t)img.w * img.h), och((size_t)w * h);
  bgr.assign((size_t)w * h * 3, 0);
  for (int k = 0; k < 3; ++k) {
    for (size_t q = 0; q < ch.size(); ++q) ch[q] = img.bgr[3 * q + k];
    resize_u8(ch.data(), img.w, img.h, och.data(), w, h);
    for (size_t q = 0; q < och.size(); ++q) bgr[3 * q + k] = och[q];
  }
  scale_intrinsics(cam, w / (float)img.w, h / (float)img.h);
}

long long depth_point_cloud(int mode, int w, int h, const float* depth, const uint8_t* weak, const DpeCamera& cam,
                            const uint8_t* bgr, float depth_min, float depth_max, FusedPoint* out, size_t cap) {
  size_t n = 0;
  for (int i = 0; i < w; ++i) {
    for (int j = 0; j < h; ++j) {
      const size_t p = (size_t)j * w + i;
      // main.cpp:464: the depth of a pixel that is not STRONG is replaced, the pixel is not dropped
      const float d = (mode == DPE_POINTS_STRONG && weak[p] != DPE_STRONG) ? 0.0f : depth[p];
      uint32_t bits;
      std::memcpy(&bits, &d, 4);
      const bool is_nan = (bits & 0x7FFFFFFFu) > 0x7F800000u;   // on the bits: no fast-math flag folds it away
      if (d < depth_min || d > depth_max || is_nan) continue;
      if (n == cap) return -1;
      const float col[3] = {(float)bgr[3 * p], (float)bgr[3 * p + 1], (float)bgr[3 * p + 2]};
      out[n++] = fusion_point(i, j, d, cam, col);
    }
  }
  return (long long)n;
}

}  // namespace dpe_host

extern "C" {

long long dpe_host_depth_point_cloud(int mode, int w, int h, const float* depth, const uint8_t* weak, const DpeCamera* cam,
                                     const uint8_t* bgr, float depth_min, float depth_max, DpeFusedPoint* out, size_t cap) {
  if ((mode != DPE_POINTS_ALL && mode != DPE_POINTS_STRONG) || w < 1 || h < 1 || !depth || !cam || !bgr || (!out && cap > 0) ||
      (mode == DPE_POINTS_STRONG && !weak))
    return -1;
  return dpe_host::depth_point_cloud(mode, w, h, depth, weak, *cam, bgr, depth_min, depth_max, out, cap);
}

int dpe_host_rescale_image_and_camera(const uint8_t* bgr, int src_w, int src_h, int w, int h, DpeCamera* cam,
                                      uint8_t* out_bgr) {
  if (!bgr || !cam || !out_bgr || src_w < 1 || src_h < 1 || w < 1 || h < 1) return 1;
  if (src_w == w && src_h == h) {
    std::memcpy(out_bgr, bgr, (size_t)w * h * 3);
    return 0;
  }
  dpe_host::ColorImage img;
  img.w = src_w; img.h = src_h;
  img.bgr.assign(bgr, bgr + (size_t)src_w * src_h * 3);
  std::vector<uint8_t> o;
  dpe_host::resize_bgr_and_camera(img, w, h, *cam, o);
  std::memcpy(out_bgr, o.data(), o.size());
  return 0;
}

int dpe_host_write_point_cloud(const char* path, const DpeFusedPoint* points, size_t n) {
  if (!path || (!points && n > 0)) return 1;
  std::string err;
  return dpe_host::export_point_cloud(path, points, n, err) ? 0 : 1;
}

}  // extern "C"
