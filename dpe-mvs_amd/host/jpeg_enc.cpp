// jpeg_enc.cpp — a baseline JPEG encoder that writes what cv::imwrite(path, mat) writes with its
// defaults (libjpeg: quality 95, baseline sequential, the Annex K Huffman tables, a JFIF APP0
// segment, 4:2:0 for 8UC3 = BGR, one component for 8UC1).  Integer arithmetic only.
//
// Split at the seam the GPU needs: the front half (pixels -> quantised coefficient blocks,
// csrc/jpeg_front.h, shared with the device kernels of csrc/pass_viz.h) and the back half here
// (DC prediction, Huffman coding, byte stuffing, headers, file).  Blocks are in scan (MCU)
// order, 64 int16 each in NATURAL order; the zigzag is applied here.
#include "host.h"

#include "../csrc/jpeg_front.h"

#include <cstdio>
#include <cstring>

namespace dpe_host {
namespace {

const uint8_t kZig[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                          41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K.3 - K.6
const uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

struct HuffEnc {
  uint16_t code[256];
  uint8_t len[256];
  void build(const uint8_t* bits, const uint8_t* vals) {   // Annex C
    std::memset(len, 0, sizeof(len));
    std::memset(code, 0, sizeof(code));
    int k = 0;
    unsigned c = 0;
    for (int l = 1; l <= 16; ++l) {
      for (int i = 0; i < bits[l - 1]; ++i, ++k) { code[vals[k]] = (uint16_t)c++; len[vals[k]] = (uint8_t)l; }
      c <<= 1;
    }
  }
};

struct BitWriter {
  std::vector<uint8_t>& out;
  uint32_t acc = 0;
  int n = 0;
  explicit BitWriter(std::vector<uint8_t>& o) : out(o) {}
  void put(unsigned code, int len) {
    if (!len) return;
    acc = (acc << len) | (code & ((1u << len) - 1u));
    n += len;
    while (n >= 8) {
      const uint8_t b = (uint8_t)(acc >> (n - 8));
      out.push_back(b);
      if (b == 0xFF) out.push_back(0);
      n -= 8;
    }
  }
  void flush() { if (n) put(0x7F, 8 - n); }   // pad with one-bits
};

int nbits_of(int v) { int n = 0; while (v) { n++; v >>= 1; } return n; }

void encode_block(BitWriter& bw, const int16_t* blk, int& last_dc, const HuffEnc& dc, const HuffEnc& ac) {
  int temp = (int)blk[0] - last_dc, temp2 = temp;
  last_dc = blk[0];
  if (temp < 0) { temp = -temp; temp2--; }
  int nb = nbits_of(temp);
  bw.put(dc.code[nb], dc.len[nb]);
  bw.put((unsigned)temp2, nb);
  int r = 0;
  for (int k = 1; k < 64; ++k) {
    temp = blk[kZig[k]];
    if (temp == 0) { r++; continue; }
    while (r > 15) { bw.put(ac.code[0xF0], ac.len[0xF0]); r -= 16; }
    temp2 = temp;
    if (temp < 0) { temp = -temp; temp2--; }
    nb = nbits_of(temp);
    const int sym = (r << 4) + nb;
    bw.put(ac.code[sym], ac.len[sym]);
    bw.put((unsigned)temp2, nb);
    r = 0;
  }
  if (r > 0) bw.put(ac.code[0], ac.len[0]);
}

void put16(std::vector<uint8_t>& o, int v) { o.push_back((uint8_t)(v >> 8)); o.push_back((uint8_t)v); }

void put_dht(std::vector<uint8_t>& o, int tc_th, const uint8_t* bits, const uint8_t* vals) {
  int n = 0;
  for (int i = 0; i < 16; ++i) n += bits[i];
  o.push_back(0xFF); o.push_back(0xC4);
  put16(o, 2 + 1 + 16 + n);
  o.push_back((uint8_t)tc_th);
  o.insert(o.end(), bits, bits + 16);
  o.insert(o.end(), vals, vals + n);
}

}  // namespace

size_t jpeg_block_count(int w, int h, int channels) {
  return (size_t)dpe_jpeg::mcus_x(w, channels) * dpe_jpeg::mcus_y(h, channels) * (channels == 3 ? 6 : 1);
}

// front half on the host: the same functions the device kernels run (csrc/jpeg_front.h)
void jpeg_blocks(const uint8_t* px, int w, int h, int channels, int quality, int16_t* blocks) {
  uint16_t q[128];
  dpe_jpeg::quant_tables(quality, q);
  const int mx_n = dpe_jpeg::mcus_x(w, channels), my_n = dpe_jpeg::mcus_y(h, channels), per = channels == 3 ? 6 : 1;
  for (int my = 0; my < my_n; ++my)
    for (int mx = 0; mx < mx_n; ++mx)
      for (int k = 0; k < per; ++k) {
        int comp, bx, by;
        bool dummy;
        dpe_jpeg::block_source(w, h, channels, mx, my, k, &comp, &bx, &by, &dummy);
        int d[64];
        for (int r = 0; r < 8; ++r) {
          for (int c = 0; c < 8; ++c) d[r * 8 + c] = dpe_jpeg::sample(px, w, h, channels, comp, bx * 8 + c, by * 8 + r);
          dpe_jpeg::fdct_1d(d + r * 8, 1);
        }
        for (int c = 0; c < 8; ++c) {
          int col[8];
          for (int r = 0; r < 8; ++r) col[r] = d[r * 8 + c];
          dpe_jpeg::fdct_1d(col, 2);
          for (int r = 0; r < 8; ++r) d[r * 8 + c] = col[r];
        }
        int16_t* o = blocks + (((size_t)my * mx_n + mx) * per + k) * 64;
        const uint16_t* qt = q + (comp ? 64 : 0);
        for (int i = 0; i < 64; ++i) o[i] = (dummy && i) ? (int16_t)0 : (int16_t)dpe_jpeg::quantise(d[i], qt[i]);
      }
}

// back half: blocks -> the JPEG file image
void jpeg_encode_blocks(const int16_t* blocks, int w, int h, int channels, int quality, std::vector<uint8_t>& o) {
  uint16_t q[128];
  dpe_jpeg::quant_tables(quality, q);
  const int nc = channels == 3 ? 3 : 1;
  o.clear();
  o.reserve(jpeg_block_count(w, h, channels) * 24 + 1024);
  o.push_back(0xFF); o.push_back(0xD8);
  const uint8_t app0[18] = {0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  o.insert(o.end(), app0, app0 + 18);
  for (int t = 0; t < (nc == 3 ? 2 : 1); ++t) {
    o.push_back(0xFF); o.push_back(0xDB);
    put16(o, 67);
    o.push_back((uint8_t)t);
    for (int i = 0; i < 64; ++i) o.push_back((uint8_t)q[t * 64 + kZig[i]]);
  }
  o.push_back(0xFF); o.push_back(0xC0);
  put16(o, 8 + 3 * nc);
  o.push_back(8);
  put16(o, h); put16(o, w);
  o.push_back((uint8_t)nc);
  for (int c = 0; c < nc; ++c) {
    o.push_back((uint8_t)(c + 1));
    o.push_back((uint8_t)((nc == 3 && c == 0) ? 0x22 : 0x11));
    o.push_back((uint8_t)(c ? 1 : 0));
  }
  HuffEnc dc[2], ac[2];
  for (int t = 0; t < (nc == 3 ? 2 : 1); ++t) {
    dc[t].build(kDcBits[t], kDcVals);
    ac[t].build(kAcBits[t], kAcVals[t]);
    put_dht(o, 0x00 | t, kDcBits[t], kDcVals);
    put_dht(o, 0x10 | t, kAcBits[t], kAcVals[t]);
  }
  o.push_back(0xFF); o.push_back(0xDA);
  put16(o, 6 + 2 * nc);
  o.push_back((uint8_t)nc);
  for (int c = 0; c < nc; ++c) { o.push_back((uint8_t)(c + 1)); o.push_back((uint8_t)(c ? 0x11 : 0x00)); }
  o.push_back(0); o.push_back(63); o.push_back(0);
  BitWriter bw(o);
  int last_dc[3] = {0, 0, 0};
  const size_t n_mcu = (size_t)dpe_jpeg::mcus_x(w, channels) * dpe_jpeg::mcus_y(h, channels);
  const int16_t* b = blocks;
  for (size_t m = 0; m < n_mcu; ++m) {
    if (nc == 3) {
      for (int k = 0; k < 4; ++k, b += 64) encode_block(bw, b, last_dc[0], dc[0], ac[0]);
      encode_block(bw, b, last_dc[1], dc[1], ac[1]); b += 64;
      encode_block(bw, b, last_dc[2], dc[1], ac[1]); b += 64;
    } else {
      encode_block(bw, b, last_dc[0], dc[0], ac[0]); b += 64;
    }
  }
  bw.flush();
  o.push_back(0xFF); o.push_back(0xD9);
}

bool jpeg_write_blocks(const std::string& path, const int16_t* blocks, int w, int h, int channels, int quality,
                       std::string& err) {
  std::vector<uint8_t> o;
  jpeg_encode_blocks(blocks, w, h, channels, quality, o);
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) { err = "cannot write " + path; return false; }
  const bool ok = std::fwrite(o.data(), 1, o.size(), f) == o.size();
  if (std::fclose(f) != 0 || !ok) { err = "cannot write " + path; return false; }
  return true;
}

bool write_jpeg(const std::string& path, const uint8_t* px, int w, int h, int channels, int quality, std::string& err) {
  std::vector<int16_t> blocks(jpeg_block_count(w, h, channels) * 64);
  jpeg_blocks(px, w, h, channels, quality, blocks.data());
  return jpeg_write_blocks(path, blocks.data(), w, h, channels, quality, err);
}

}  // namespace dpe_host

extern "C" {

static bool jpeg_args_ok(int w, int h, int channels, int quality) {
  return w >= 1 && h >= 1 && w <= 65535 && h <= 65535 && (channels == 1 || channels == 3) && quality >= 1 && quality <= 100;
}

int dpe_host_jpeg_blocks(const uint8_t* pixels, int w, int h, int channels, int quality, int16_t* blocks, size_t cap,
                         size_t* n_blocks) {
  if (!jpeg_args_ok(w, h, channels, quality)) return 1;
  const size_t n = dpe_host::jpeg_block_count(w, h, channels);
  if (n_blocks) *n_blocks = n;
  if (!blocks) return 0;
  if (!pixels) return 1;
  if (cap < n * 64) return 2;
  dpe_host::jpeg_blocks(pixels, w, h, channels, quality, blocks);
  return 0;
}

int dpe_host_jpeg_write_blocks(const char* path, const int16_t* blocks, int w, int h, int channels, int quality) {
  if (!path || !blocks || !jpeg_args_ok(w, h, channels, quality)) return 1;
  std::string err;
  return dpe_host::jpeg_write_blocks(path, blocks, w, h, channels, quality, err) ? 0 : 1;
}

int dpe_host_write_jpeg(const char* path, const uint8_t* pixels, int w, int h, int channels, int quality) {
  if (!path || !pixels || !jpeg_args_ok(w, h, channels, quality)) return 1;
  std::string err;
  return dpe_host::write_jpeg(path, pixels, w, h, channels, quality, err) ? 0 : 1;
}

}  // extern "C"
