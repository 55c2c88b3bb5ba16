// dpe_fusion_types.h -- the plain structs the fusion kernels (pass_fusion.h, pass_fusion_tat.h) share
// with the context that stages them (dpe_context.h), apart from the kernels so that the context does
// not depend on a kernel header.
#pragma once
#include <stdint.h>

namespace dpe {

struct FusionViewDev {
  const float* depth;
  const float* normal;
  int w, h;
};

struct TatViewDev {
  const uint8_t* bgr;      // [H][W][3]
  const uint8_t* block;    // [H][W] or nullptr
  uint8_t* mask;           // [H][W] fusion mask
};
struct TatPoint { float x, y, z, b, g, r; };

}  // namespace dpe
