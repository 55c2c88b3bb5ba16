"""The fast taps' texel offset (dpe-mvs_amd/csrc/tex_addr.h), compiled with g++: the two-instruction
form (byte permute + 16-bit dot product) against the four-instruction form it replaces and against
the plain offset vofs + (Y * stride + X) * bytes, modulo 2^32, for every pair of clamped coordinate
encodings of a frame.

  * all three 8-bit / quarter-integer layouts, frames from 1x1 to the widest the 8-byte layout takes
    (W = 8189), the first it does not (8190) and 16382 (past dpe_pm_stage's 16000 limit, where the
    4-byte layouts' rows pass 65535 bytes as well), view offsets of views 0, 1 and 31;
  * each texel index with the smallest and the largest weight byte under it (the offset ignores it);
  * the host's per-pass predicate says "wide" exactly where a row of texels passes 65535 bytes, and
    there the four-instruction form still equals the plain offset.
"""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "dpe-mvs_amd", "csrc", "tex_addr.h")
LAYOUTS = {"TEX_U8": 1, "TEX_F16": 2, "TEX_P16": 3}
BYTES = {"TEX_U8": 4, "TEX_F16": 8, "TEX_P16": 4}
PAD = {"TEX_U8": 2, "TEX_F16": 2, "TEX_P16": 3}          # row stride = W + PAD texels
FRAMES = [(1, 1), (2, 3), (64, 48), (1600, 1200), (8189, 3), (8190, 3), (16382, 2)]
VIEWS = [0, 1, 31]

SRC = r'''
#include "%s"
using namespace dpe;
// encodings of texel index X with weight byte f: bits(1.5 * 2^15) + 256 X + f
static uint32_t enc(uint32_t X, uint32_t f) { return 0x47400000u + 256u * X + f; }
// mismatches over X in 0..W+1, Y = y0, y0 + ystep, .. <= H+1; which: 0 two-instruction form against the
// four-instruction one, 1 four-instruction form against the plain offset, 2 packed fields
template <int T> static long sweep(int W, int H, int y0, int ystep, uint32_t vofs, int which) {
  const uint32_t stride = tex_stride<T>(W);
  const uint32_t coef = tex_coef<T>(stride), vadj2 = tex_vadj2<T>(vofs, stride), vadj = tex_vadj<T>(vofs, stride);
  long bad = 0;
  for (uint32_t Y = y0; Y <= (uint32_t)H + 1; Y += ystep)
    for (uint32_t X = 0; X <= (uint32_t)W + 1; ++X)
      for (uint32_t f = 0; f < 256; f += 255) {
        const uint32_t by = enc(Y, 255 - f), bx = enc(X, f);
        const uint32_t four = tex_offset4<T>(by, bx, stride, vadj);
        if (which == 0) bad += tex_offset2(tex_pack(by, bx), coef, vadj2) != four;
        else if (which == 1) bad += four != vofs + (Y * stride + X) * tex_bytes<T>();
        else bad += tex_pack(by, bx) != ((0x4000u + Y) << 16 | (0x4000u + X));
      }
  return bad;
}
extern "C" long sweep_layout(int T, int W, int H, int y0, int ystep, uint32_t vofs, int which) {
  return T == TEX_U8 ? sweep<TEX_U8>(W, H, y0, ystep, vofs, which)
       : T == TEX_F16 ? sweep<TEX_F16>(W, H, y0, ystep, vofs, which) : sweep<TEX_P16>(W, H, y0, ystep, vofs, which);
}
extern "C" int wide(int T, int W) {
  return T == TEX_U8 ? tex_wide<TEX_U8>(W) : T == TEX_F16 ? tex_wide<TEX_F16>(W) : tex_wide<TEX_P16>(W);
}
extern "C" uint32_t stride_of(int T, int W) {
  return T == TEX_U8 ? tex_stride<TEX_U8>(W) : T == TEX_F16 ? tex_stride<TEX_F16>(W) : tex_stride<TEX_P16>(W);
}
extern "C" uint32_t bytes_of(int T) { return T == TEX_F16 || T == TEX_F16W ? 8 : 4; }
extern "C" int f16w_is_f16() { return tex_bytes<TEX_F16W>() == tex_bytes<TEX_F16>() && tex_stride<TEX_F16W>(7) == tex_stride<TEX_F16>(7); }
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("tex_addr")
    src = d / "t.cpp"
    src.write_text(SRC % HDR)
    so = d / "t.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)], check=True)
    L = C.CDLL(str(so))
    L.sweep_layout.restype = C.c_long
    L.sweep_layout.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int]
    L.stride_of.restype = C.c_uint32
    L.bytes_of.restype = C.c_uint32
    return L


def _view_bytes(name, W, H):
    return (W + PAD[name]) * (H + 2) * BYTES[name]


def _rows(W, H):
    """(first row, step) sweeps of a frame: every row, but of 1600x1200 every 7th and the last three"""
    return [(0, 7), (H - 1, 1)] if (W, H) == (1600, 1200) else [(0, 1)]


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_layout_constants(lib, name):
    T = LAYOUTS[name]
    assert lib.bytes_of(T) == BYTES[name]
    for W in (1, 64, 1600, 16382):
        assert lib.stride_of(T, W) == W + PAD[name]
    assert lib.f16w_is_f16() == 1


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_wide_predicate(lib, name):
    T = LAYOUTS[name]
    for W in range(1, 16384):
        assert bool(lib.wide(T, W)) == ((W + PAD[name]) * BYTES[name] > 65535), (name, W)
    # the 8-byte layout from W = 8190 on; the 4-byte ones at no width dpe_pm_stage accepts (16000),
    # though at 16382 their rows pass 65535 bytes too (65536 and 65540)
    assert not lib.wide(T, 8189)
    assert bool(lib.wide(T, 8190)) == (name == "TEX_F16")
    assert bool(lib.wide(T, 16000)) == (name == "TEX_F16")
    assert lib.wide(T, 16382)


@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_offsets_equal(lib, name, W, H):
    T = LAYOUTS[name]
    wide = (W + PAD[name]) * BYTES[name] > 65535
    assert bool(lib.wide(T, W)) == wide
    for v in VIEWS:
        vofs = v * _view_bytes(name, W, H)
        assert vofs + _view_bytes(name, W, H) < 2 ** 32
        for y0, ystep in _rows(W, H):
            assert lib.sweep_layout(T, W, H, y0, ystep, vofs, 2) == 0, (name, W, H, v, "packed fields")
            # the definition itself: today's four-instruction form is the plain offset, wide or not
            assert lib.sweep_layout(T, W, H, y0, ystep, vofs, 1) == 0, (name, W, H, v, "four-instruction form")
            bad = lib.sweep_layout(T, W, H, y0, ystep, vofs, 0)
            if wide:
                assert bad > 0, (name, W, H, v, "the predicate is there for a reason")
            else:
                assert bad == 0, (name, W, H, v, "two-instruction form")
