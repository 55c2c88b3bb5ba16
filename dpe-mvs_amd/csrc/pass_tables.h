// pass_tables.h — pass-constant tables the host fills once per pass (PassConst::base_len, ::spat36).
//
// Both hold float expressions the kernels used to evaluate per pixel.  The library is built with
// -ffp-contract=off, and sqrtf and / are correctly rounded on the host as on gfx950, so the same
// expression written here gives the bits the device computed.  Plain C++ (no HIP): the CPU tests
// compile this header with g++ and compare it with a float32 restatement.
#pragma once
#include <math.h>

namespace dpe {

constexpr int kSpatTaps = 36;   // the 6 x 6 taps of the default Old-NCC patch (radius 5, increment 2)

// Spatial term of ComputeBilateralWeight (DPE.cu:550-555) for tap k = a * 6 + b of the 5/2 patch,
// offsets (i, j) = (-5 + 2a, -5 + 2b): -sqrt(i^2 + j^2) / (2 sigma_spatial^2), with `sd` as in
// bilateral_weight (pass_common.h).  The weight is then d_expf(spat36[k] - cd / (2 sc sc)).
inline void build_spat36(float ss, float* spat36) {
  for (int k = 0; k < kSpatTaps; ++k) {
    const float xd = (float)(-5 + 2 * (k / 6)), yd = (float)(-5 + 2 * (k % 6));
    const float sd = sqrtf(xd * xd + yd * yd);
    spat36[k] = -sd / (2.0f * ss * ss);
  }
}

// Length of the baseline between the reference camera centre c0 and a source camera centre cs
// (within DPE.cu:2629-2648), the summand of baseline_and_weights (pass_refine.h).
inline float baseline_length(const float* c0, const float* cs) {
  const float d0 = c0[0] - cs[0], d1 = c0[1] - cs[1], d2 = c0[2] - cs[2];
  const float tv = d0 * d0 + d1 * d1 + d2 * d2;
  return sqrtf(tv);
}

}  // namespace dpe
