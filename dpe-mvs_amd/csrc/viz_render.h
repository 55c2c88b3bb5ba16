// viz_render.h — the per-pixel rules of the reference's medium-result pictures (ShowDepthMap,
// ShowNormalMap, ShowWeakImage, DPE.cpp:384-502), shared by the host renderer (host/viz.cpp) and
// the device kernel (pass_viz.h): the same function compiles for both.  Single precision except
// where the reference promotes (the double square root of the normal's length, the two double
// expressions of the depth ramp's last segments); the build sets -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DPE_VHD __host__ __device__ __forceinline__
#else
#define DPE_VHD inline
#endif

namespace dpe_viz {

enum { KIND_DEPTH = 0, KIND_NORMAL = 1, KIND_WEAK = 2 };

// ShowDepthMap (DPE.cpp:391-442): black outside [dmin, dmax] or NaN, else the five-segment ramp
DPE_VHD void depth_px(float d, float dmin, float dmax, uint8_t* bgr) {
  bgr[0] = bgr[1] = bgr[2] = 0;
  if (d < dmin || d > dmax || d != d) return;
  float v = (dmax - d) / (dmax - dmin);
  if (v > 1) v = 1;
  if (v < 0) v = 0;
  v = v * 255;
  if (v > 255) v = 255;
  else if (v < 0) v = 0;
  if (v <= 51) { bgr[0] = 255; bgr[1] = (uint8_t)(int)(v * 5); }
  else if (v <= 102) { v -= 51; bgr[0] = (uint8_t)(int)(255 - v * 5); bgr[1] = 255; }
  else if (v <= 153) { v -= 102; bgr[1] = 255; bgr[2] = (uint8_t)(int)(v * 5); }
  else if (v <= 204) { v -= 153; bgr[1] = (uint8_t)(255 - (int)(uint8_t)(int)((double)v * 128.0 / 51 + 0.5)); bgr[2] = 255; }
  else if (v <= 255) { v -= 204; bgr[1] = (uint8_t)(127 - (int)(uint8_t)(int)((double)v * 127.0 / 51 + 0.5)); bgr[2] = 255; }
}

// cv::saturate_cast<uchar>(float): round half to even, clamp; NaN -> 0
DPE_VHD uint8_t sat_round_u8(float v) {
  const float t = rintf(v);
  if (!(t >= 0.0f)) return 0;
  return t > 255.0f ? (uint8_t)255 : (uint8_t)(int)t;
}

// ShowNormalMap (DPE.cpp:455-470): normalise (length in double), then convertTo(8U, 127.5, 127.5)
DPE_VHD void normal_px(float x, float y, float z, uint8_t* bgr) {
  const float norm = (float)sqrt((double)x * (double)x + (double)y * (double)y + (double)z * (double)z);
  if (norm == 0) { x = y = z = 0.0f; }
  else { const float s = 1.f / norm; x = x * s; y = y * s; z = z * s; }
  bgr[0] = sat_round_u8(x * 127.5f + 127.5f);
  bgr[1] = sat_round_u8(y * 127.5f + 127.5f);
  bgr[2] = sat_round_u8(z * 127.5f + 127.5f);
}

// ShowWeakImage (DPE.cpp:485-496); a value outside the enum is left black
DPE_VHD void weak_px(uint8_t s, uint8_t* bgr) {
  bgr[0] = bgr[1] = bgr[2] = 0;
  if (s == 0) { bgr[0] = bgr[1] = bgr[2] = 255; }   // WEAK
  else if (s == 1) bgr[1] = 255;                    // STRONG
  else if (s == 2) bgr[2] = 255;                    // UNKNOWN
}

}  // namespace dpe_viz
