// tex_addr.h — the byte offset of a fast tap's quad texel, straight from its two coordinate encodings.
//
// A clamped tap coordinate t lies in [1.5 * 2^15, 2^16) on the 1/256 grid, so its encoding is
//   bits(t) = 0x47400000 + U,  U = 256 X + weight,  X = the texel index, 0 .. lim + 1 < 0x4000
// (pass_common.h "tap coordinates").  The texel (X, Y) of view offset vofs in a layout of `bytes`
// per texel and `stride` texels per row is at
//   offset = vofs + (Y * stride + X) * bytes                                   (below 2^32)
// Two forms compute it from bits(ty), bits(tx), both modulo 2^32 with the encodings' constant part
// folded into the view offset:
//
//  * tex_offset4, four instructions (two shifts, v_mad_u32_u24, v_lshl_add_u32), any stride:
//      offset = vadj + (umul24(bits(ty) >> 8, stride) + (bits(tx) >> 8)) * bytes
//      vadj   = vofs - 0x474000 * (stride + 1) * bytes           (bits(t) >> 8 = 0x474000 + X < 2^24)
//    This is the definition the other form must equal.
//
//  * tex_offset2, two instructions (v_perm_b32, v_dot2_u32_u16), stride * bytes <= 65535:
//      packed = {bits(ty).byte2, bits(ty).byte1, bits(tx).byte2, bits(tx).byte1}
//             = two 16-bit fields (0x4000 + Y, 0x4000 + X): no carry out of a field while X < 0xC000
//      offset = vadj2 + lo16(packed) * bytes + hi16(packed) * (stride * bytes)
//      vadj2  = vofs - 0x4000 * (bytes + stride * bytes)
//    tex_wide says where the row coefficient no longer fits 16 bits (the 8-byte layout from
//    W = 8190 on); such a pass uses tex_offset4.
//
// Plain C++ under a host compiler (the CPU tests compile it with g++), the two builtins on the device.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define TEX_HD __host__ __device__ __forceinline__
#else
#define TEX_HD inline
#endif

namespace dpe {

// Source-image layouts (pass_common.h describes their texels).  TEX_F16W is TEX_F16's texels
// addressed with tex_offset4: the instantiation of a pass whose frames are tex_wide.
enum { TEX_F32 = 0, TEX_U8 = 1, TEX_F16 = 2, TEX_P16 = 3, TEX_F16W = 4 };
template <int T> constexpr uint32_t tex_bytes() { return T == TEX_F16 || T == TEX_F16W ? 8u : 4u; }
template <int T> TEX_HD constexpr uint32_t tex_stride(int W) { return (uint32_t)(W + (T == TEX_P16 ? 3 : 2)); }

constexpr uint32_t kTexMagicHi = 0x474000u;   // bits(1.5 * 2^15) >> 8: texel index bias of bits(t) >> 8
constexpr uint32_t kTexMagic16 = 0x4000u;     // its low 16 bits: texel index bias of a packed field

// ---- four-instruction form
template <int T> TEX_HD uint32_t tex_vadj(uint32_t vofs, uint32_t stride) {
  return vofs - kTexMagicHi * (stride + 1u) * tex_bytes<T>();
}
template <int T> TEX_HD uint32_t tex_offset4(uint32_t bits_ty, uint32_t bits_tx, uint32_t stride, uint32_t vadj) {
#if defined(__HIP_DEVICE_COMPILE__)
  return vadj + (__umul24(bits_ty >> 8, stride) + (bits_tx >> 8)) * tex_bytes<T>();
#else
  return vadj + (((bits_ty >> 8) & 0xFFFFFFu) * (stride & 0xFFFFFFu) + (bits_tx >> 8)) * tex_bytes<T>();
#endif
}

// ---- two-instruction form
// true when layout T's row coefficient of a W-pixel-wide frame does not fit the 16-bit field
template <int T> TEX_HD constexpr bool tex_wide(int W) { return tex_stride<T>(W) * tex_bytes<T>() > 65535u; }
// (0x4000 + Y) << 16 | (0x4000 + X)
TEX_HD uint32_t tex_pack(uint32_t bits_ty, uint32_t bits_tx) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(bits_ty, bits_tx, 0x06050201u);
#else
  return ((bits_ty >> 8) & 0xFFFFu) << 16 | ((bits_tx >> 8) & 0xFFFFu);
#endif
}
// {stride * bytes, bytes}; only for !tex_wide
template <int T> TEX_HD uint32_t tex_coef(uint32_t stride) { return (stride * tex_bytes<T>()) << 16 | tex_bytes<T>(); }
template <int T> TEX_HD uint32_t tex_vadj2(uint32_t vofs, uint32_t stride) {
  return vofs - (stride + 1u) * (kTexMagic16 * tex_bytes<T>());
}
TEX_HD uint32_t tex_offset2(uint32_t packed, uint32_t coef, uint32_t vadj2) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  return __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, packed), __builtin_bit_cast(u16x2, coef), vadj2, false);
#else
  return vadj2 + (packed & 0xFFFFu) * (coef & 0xFFFFu) + (packed >> 16) * (coef >> 16);
#endif
}

}  // namespace dpe
