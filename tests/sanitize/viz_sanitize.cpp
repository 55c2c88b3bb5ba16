// Drives the JPEG encoder (host/jpeg_enc.cpp) and the viz renderers (host/viz.cpp) under ASan +
// UBSan (tests/test_viz.py): every buffer is a heap allocation of exactly the size the function is
// given, so a read or write past an image, block or picture buffer is reported.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "../../include/dpe_host.h"

static int fail(const char* what, int w, int h) {
  std::fprintf(stderr, "viz sanitize: %s failed at %dx%d\n", what, w, h);
  return 1;
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  const int sizes[4][2] = {{1, 1}, {7, 3}, {17, 9}, {16, 16}};
  for (const auto& sz : sizes) {
    const int w = sz[0], h = sz[1];
    const size_t L = (size_t)w * h;
    std::vector<float> depth(L), normal(L * 3);
    std::vector<uint8_t> weak(L);
    for (size_t i = 0; i < L; ++i) {
      depth[i] = i % 7 == 0 ? std::numeric_limits<float>::quiet_NaN() : 0.5f + 0.37f * (float)(i % 11);
      normal[3 * i] = (float)(i % 5) - 2.0f;
      normal[3 * i + 1] = i % 9 == 0 ? std::numeric_limits<float>::quiet_NaN() : 0.25f * (float)(i % 3);
      normal[3 * i + 2] = i % 4 == 0 ? 0.0f : -1.5f;
      weak[i] = (uint8_t)(i % 4);
    }
    for (int channels : {3, 1}) {
      size_t n = 0;
      if (dpe_host_jpeg_blocks(nullptr, w, h, channels, 95, nullptr, 0, &n) != 0) return fail("size query", w, h);
      std::vector<int16_t> blocks(n * 64);
      std::vector<uint8_t> px(L * channels);
      for (int kind = 0; kind < 3; ++kind) {
        if (channels == 3) {
          if (dpe_host_viz_render(kind, w, h, kind == DPE_VIZ_DEPTH ? depth.data() : nullptr,
                                  kind == DPE_VIZ_NORMAL ? normal.data() : nullptr, kind == DPE_VIZ_WEAK ? weak.data() : nullptr,
                                  1.0f, 4.0f, px.data()) != 0)
            return fail("render", w, h);
        } else {
          for (size_t i = 0; i < L; ++i) px[i] = (i * 37 + kind) % 3 == 0 ? 255 : 0;
        }
        if (dpe_host_jpeg_blocks(px.data(), w, h, channels, 95, blocks.data(), blocks.size(), &n) != 0) return fail("blocks", w, h);
        const std::string path = dir + "/viz_" + std::to_string(w) + "x" + std::to_string(h) + "_" + std::to_string(channels) +
                                 "_" + std::to_string(kind) + ".jpg";
        if (dpe_host_jpeg_write_blocks(path.c_str(), blocks.data(), w, h, channels, 95) != 0) return fail("write blocks", w, h);
        if (dpe_host_write_jpeg(path.c_str(), px.data(), w, h, channels, 95) != 0) return fail("write", w, h);
      }
      // extreme coefficients: a checkerboard of 0 / 255 at quality 100
      for (size_t i = 0; i < px.size(); ++i) px[i] = ((i / channels) % w + (i / channels) / w) % 2 ? 255 : 0;
      if (dpe_host_jpeg_blocks(px.data(), w, h, channels, 100, blocks.data(), blocks.size(), &n) != 0) return fail("blocks q100", w, h);
      const std::string path = dir + "/viz_q100.jpg";
      if (dpe_host_jpeg_write_blocks(path.c_str(), blocks.data(), w, h, channels, 100) != 0) return fail("write q100", w, h);
    }
  }
  std::printf("viz sanitize ok\n");
  return 0;
}
