// jpeg_front.h — the data-parallel ("front") half of the baseline JPEG encoder, as integer
// arithmetic shared by the host encoder (host/jpeg_enc.cpp) and the device kernels (pass_viz.h):
// the same functions compile for both, so the two are bit-identical by construction.
//
// What it restates is libjpeg's published algorithm for cv::imwrite's defaults (quality 95,
// baseline, 4:2:0): the 16-bit fixed-point RGB -> YCbCr conversion, h2v2 chroma averaging with
// the alternating 1, 2 bias, edge replication, the level shift, the "islow" Loeffler-Ligtenberg-
// Moschytz forward DCT (13-bit constants, 2 pass-1 bits, output scaled by 8) and quantisation by
// 8 * q with rounding half away from zero.  tests/test_viz.py pins it against libjpeg through PIL.
//
// Block layout (both halves): per MCU the blocks Y00 Y01 Y10 Y11 Cb Cr (colour, 16x16 MCUs,
// MCUs in raster order) or one Y block (grey, 8x8 MCUs); 64 int16 coefficients per block in
// NATURAL (row-major, v * 8 + u) order -- the back half applies the zigzag.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DPE_JHD __host__ __device__ __forceinline__
#else
#define DPE_JHD inline
#endif

namespace dpe_jpeg {

// Annex K.1 / K.2 base tables, natural order (host only: the kernels get the scaled tables)
inline int base_q(int chroma, int i) {
  const uint8_t luma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                            14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                            18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                            49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
  const uint8_t chrom[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
                             24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                             99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                             99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
  return chroma ? chrom[i] : luma[i];
}

// jpeg_quality_scaling + jpeg_add_quant_table(force_baseline): q[0..63] luma, q[64..127] chroma
inline void quant_tables(int quality, uint16_t* q) {
  if (quality < 1) quality = 1;
  if (quality > 100) quality = 100;
  const int scale = quality < 50 ? 5000 / quality : 200 - quality * 2;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) {
      int v = (base_q(t, i) * scale + 50) / 100;
      if (v < 1) v = 1;
      if (v > 255) v = 255;
      q[t * 64 + i] = (uint16_t)v;
    }
}

// rgb_ycc_convert: comp 0 = Y, 1 = Cb, 2 = Cr (16-bit fixed point, rounding)
DPE_JHD int ycc(int comp, int r, int g, int b) {
  if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// component `comp` of the pixel (x, y) with the right / bottom edges replicated
DPE_JHD int pixel_comp(const uint8_t* px, int w, int h, int channels, int comp, int x, int y) {
  x = x < w ? x : w - 1;
  y = y < h ? y : h - 1;
  const uint8_t* p = px + ((size_t)y * w + x) * channels;
  if (channels == 1) return p[0];
  return ycc(comp, p[2], p[1], p[0]);   // 8UC3 is BGR
}

// the level-shifted sample (sx, sy) of component `comp` on its own grid: Y (and grey) full size,
// Cb / Cr h2v2-averaged with bias 1 on even, 2 on odd output columns
DPE_JHD int sample(const uint8_t* px, int w, int h, int channels, int comp, int sx, int sy) {
  if (comp == 0) return pixel_comp(px, w, h, channels, 0, sx, sy) - 128;
  // libjpeg pads the right edge before downsampling (clamped source columns) but the bottom edge
  // after it: rows below the last chroma row repeat that row, not the last source row
  const int ch = (h + 1) / 2;
  sy = sy < ch ? sy : ch - 1;
  const int s = pixel_comp(px, w, h, channels, comp, 2 * sx, 2 * sy) + pixel_comp(px, w, h, channels, comp, 2 * sx + 1, 2 * sy) +
                pixel_comp(px, w, h, channels, comp, 2 * sx, 2 * sy + 1) +
                pixel_comp(px, w, h, channels, comp, 2 * sx + 1, 2 * sy + 1);
  return ((s + 1 + (sx & 1)) >> 2) - 128;
}

DPE_JHD int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one 1-D pass of jpeg_fdct_islow over d[0..7] in place; pass 1 = rows (results scaled up by
// 2^PASS1_BITS), pass 2 = columns (PASS1_BITS removed, the factor 8 left in)
DPE_JHD void fdct_1d(int* d, int pass) {
  const int CB = 13, P1 = 2;
  const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
  const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  const int sh = pass == 1 ? CB - P1 : CB + P1;
  if (pass == 1) {
    d[0] = (tmp10 + tmp11) * (1 << P1);
    d[4] = (tmp10 - tmp11) * (1 << P1);
  } else {
    d[0] = descale(tmp10 + tmp11, P1);
    d[4] = descale(tmp10 - tmp11, P1);
  }
  int z1 = (tmp12 + tmp13) * 4433;
  d[2] = descale(z1 + tmp13 * 6270, sh);
  d[6] = descale(z1 + tmp12 * (-15137), sh);
  z1 = tmp4 + tmp7;
  int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int z5 = (z3 + z4) * 9633;
  const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
  z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
  z3 += z5; z4 += z5;
  d[7] = descale(t4 + z1 + z3, sh);
  d[5] = descale(t5 + z2 + z4, sh);
  d[3] = descale(t6 + z2 + z3, sh);
  d[1] = descale(t7 + z1 + z4, sh);
}

// quantisation of a DCT output (scaled by 8) by table entry q: divide by 8 * q, half away from zero
DPE_JHD int quantise(int coef, int q) {
  const int qv = q << 3;
  return coef < 0 ? -((-coef + (qv >> 1)) / qv) : (coef + (qv >> 1)) / qv;
}

// MCU grid and block count of a w x h image
DPE_JHD int mcus_x(int w, int channels) { return channels == 3 ? (w + 15) / 16 : (w + 7) / 8; }
DPE_JHD int mcus_y(int h, int channels) { return channels == 3 ? (h + 15) / 16 : (h + 7) / 8; }

// Which samples block `k` (0..5 colour, 0 grey) of MCU (mx, my) is computed from: component and
// the block's position on the component's grid.  A Y block that lies wholly outside the image's
// block grid is libjpeg's dummy block: every AC zero, DC that of the block before it in the MCU;
// *dummy is set and (bx, by) is the real block whose DC it carries.
DPE_JHD void block_source(int w, int h, int channels, int mx, int my, int k, int* comp, int* bx, int* by, bool* dummy) {
  *dummy = false;
  if (channels != 3) { *comp = 0; *bx = mx; *by = my; return; }
  if (k >= 4) { *comp = k - 3; *bx = mx; *by = my; return; }
  *comp = 0;
  const int ybw = (w + 7) / 8, ybh = (h + 7) / 8;
  const int cx = k & 1, cy = k >> 1;
  const bool col1 = 2 * mx + 1 < ybw, row_real = 2 * my + cy < ybh, col_real = 2 * mx + cx < ybw;
  int ux = cx, uy = cy;
  if (!row_real) { uy = 0; ux = col1 ? 1 : 0; *dummy = true; }
  else if (!col_real) { ux = 0; *dummy = true; }
  *bx = 2 * mx + ux;
  *by = 2 * my + uy;
}

}  // namespace dpe_jpeg
