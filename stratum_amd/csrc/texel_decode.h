// texel_decode.h — one texel of a source image in an asset's own format, decoded to four binary32 channels: the contract of
// include/sthip.h (sthip_texel_format), host and device from one text. Used by k_decode_texels (texel_decode.hip) and by the
// generic kernels of the material conversion (material_convert.hip).
#pragma once

#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/sthip_detmath.h"
#include "material_convert.h"

namespace sthip {

struct Texel4 {
  float x, y, z, w;
};

// ---- what a format is (sthip_texel_format; 0 and 1 are the four-channel forms here) ----
STHIP_CONVERT_HD inline uint32_t texel_canonical(uint32_t f) { return f == 0 ? (uint32_t)STHIP_TEXEL_RGBA32F_ : f == 1 ? (uint32_t)STHIP_TEXEL_RGBA8_UNORM_ : f; }
STHIP_CONVERT_HD inline bool texel_format_built(uint32_t f) { return f <= 1 || (f >= STHIP_TEXEL_FIRST && f < STHIP_TEXEL_END); }
STHIP_CONVERT_HD inline bool texel_format_named_unsupported(uint32_t f) { return f >= STHIP_TEXEL_UNSUPPORTED_FIRST && f < STHIP_TEXEL_UNSUPPORTED_END && f != 54 && f != 55; }
// the functions below take a canonical format (16 .. 39)
STHIP_CONVERT_HD inline bool texel_is_block(uint32_t f) { return f >= STHIP_TEXEL_BC1_RGB; }
STHIP_CONVERT_HD inline uint32_t texel_class(uint32_t f) { return (f - 16u) >> 2; }  // linear: 0 unorm8, 1 sRGB8, 2 unorm16, 3 binary32
STHIP_CONVERT_HD inline uint32_t texel_channels(uint32_t f) { return ((f - 16u) & 3u) + 1u; }
STHIP_CONVERT_HD inline uint32_t texel_component_bytes(uint32_t f) { return texel_class(f) < 2 ? 1u : texel_class(f) == 2 ? 2u : 4u; }
STHIP_CONVERT_HD inline uint32_t texel_block_bytes(uint32_t f) { return (f == STHIP_TEXEL_BC1_RGB || f == STHIP_TEXEL_BC1_RGB_SRGB || f == STHIP_TEXEL_BC4_UNORM) ? 8u : 16u; }
STHIP_CONVERT_HD inline bool texel_is_srgb(uint32_t f) { return texel_is_block(f) ? f >= STHIP_TEXEL_BC1_RGB_SRGB : texel_class(f) == 1; }
STHIP_CONVERT_HD inline uint32_t texel_alignment(uint32_t f) { return texel_is_block(f) ? texel_block_bytes(f) : texel_component_bytes(f); }
STHIP_CONVERT_HD inline uint64_t texel_image_bytes(uint32_t f, uint32_t w, uint32_t h) {
  if (texel_is_block(f)) return (uint64_t)((w + 3u) / 4u) * ((h + 3u) / 4u) * texel_block_bytes(f);
  return (uint64_t)w * h * texel_channels(f) * texel_component_bytes(f);
}
inline const char* texel_unsupported_name(uint32_t f) {
  static const char* const bc[] = {"BC4_SNORM", "BC5_SNORM", "BC6H_UFLOAT", "BC6H_SFLOAT", "BC7_UNORM", "BC7_SRGB"};
  if (f < 54) return bc[f - 48];
  if (f < 60) return "an 8-bit SNORM format";
  if (f < 64) return "a 16-bit SNORM format";
  return "an integer or 64-bit format";
}

// ---- the arithmetic ----
STHIP_CONVERT_HD inline float srgb_to_linear(float c) { return c <= 0.04045f ? c / 12.92f : det_powf((c + 0.055f) / 1.055f, 2.4f); }
STHIP_CONVERT_HD inline float texel_saturate(float a) { return a > 0.0f ? (a < 1.0f ? a : 1.0f) : 0.0f; }
STHIP_CONVERT_HD inline uint32_t texel_quantise(float v) { return (uint32_t)(texel_saturate(v) * 255.0f + 0.5f); }
STHIP_CONVERT_HD inline float decode_unorm16(uint32_t v) { return (float)v / 65535.0f; }

// One channel of a colour block: e0, e1 the integer endpoints, top = 31 or 63.
STHIP_CONVERT_HD inline float bc_colour_channel(uint32_t e0, uint32_t e1, float top, uint32_t index, bool four) {
  if (index == 0) return (float)e0 / top;
  if (index == 1) return (float)e1 / top;
  if (four) return index == 2 ? (float)(2u * e0 + e1) / (3.0f * top) : (float)(e0 + 2u * e1) / (3.0f * top);  // (3 * 31 = 93, 3 * 63 = 189: exact)
  return index == 2 ? (float)(e0 + e1) / (2.0f * top) : 0.0f;
}
// Texel t of the colour block in the 64-bit little-endian word `b`; BC1 decides the rule by its endpoints, BC2 / BC3 never.
STHIP_CONVERT_HD inline void bc_colour(uint64_t b, uint32_t t, bool bc1, float& r, float& g, float& bl) {
  const uint32_t c0 = (uint32_t)b & 0xFFFFu, c1 = (uint32_t)(b >> 16) & 0xFFFFu, index = (uint32_t)(b >> (32u + 2u * t)) & 3u;
  const bool four = !bc1 || c0 > c1;
  r = bc_colour_channel(c0 >> 11, c1 >> 11, 31.0f, index, four);
  g = bc_colour_channel((c0 >> 5) & 63u, (c1 >> 5) & 63u, 63.0f, index, four);
  bl = bc_colour_channel(c0 & 31u, c1 & 31u, 31.0f, index, four);
}
// Texel t of an RGTC block (BC4, the alpha of BC3, a half of BC5).
STHIP_CONVERT_HD inline float bc_rgtc(uint64_t b, uint32_t t) {
  const uint32_t r0 = (uint32_t)b & 0xFFu, r1 = (uint32_t)(b >> 8) & 0xFFu, i = (uint32_t)(b >> (16u + 3u * t)) & 7u;
  if (i == 0) return decode_unorm8(r0);
  if (i == 1) return decode_unorm8(r1);
  if (r0 > r1) return (float)((8u - i) * r0 + (i - 1u) * r1) / 1785.0f;
  if (i < 6) return (float)((6u - i) * r0 + (i - 1u) * r1) / 1275.0f;
  return i == 6 ? 0.0f : 1.0f;
}

// Texel t = 4 * (y % 4) + (x % 4) of a block whose first 8 bytes are `lo` and, for a 16-byte block, whose last 8 are `hi`.
STHIP_CONVERT_HD inline Texel4 decode_block_texel(uint32_t f, uint64_t lo, uint64_t hi, uint32_t t) {
  Texel4 v = {0.0f, 0.0f, 0.0f, 1.0f};
  switch (f) {
    case STHIP_TEXEL_BC1_RGB:
    case STHIP_TEXEL_BC1_RGB_SRGB:
      bc_colour(lo, t, true, v.x, v.y, v.z);
      break;
    case STHIP_TEXEL_BC2:
    case STHIP_TEXEL_BC2_SRGB:
      bc_colour(hi, t, false, v.x, v.y, v.z);
      v.w = (float)((uint32_t)(lo >> (4u * t)) & 15u) / 15.0f;
      break;
    case STHIP_TEXEL_BC3:
    case STHIP_TEXEL_BC3_SRGB:
      bc_colour(hi, t, false, v.x, v.y, v.z);
      v.w = bc_rgtc(lo, t);
      break;
    case STHIP_TEXEL_BC4_UNORM:
      v.x = bc_rgtc(lo, t);
      break;
    default:  // STHIP_TEXEL_BC5_UNORM
      v.x = bc_rgtc(lo, t);
      v.y = bc_rgtc(hi, t);
      break;
  }
  if (f >= STHIP_TEXEL_BC1_RGB_SRGB) v.x = srgb_to_linear(v.x), v.y = srgb_to_linear(v.y), v.z = srgb_to_linear(v.z);
  return v;
}

// Texel i of a linear image (f: 16 .. 31).
STHIP_CONVERT_HD inline Texel4 decode_linear_texel(uint32_t f, const void* base, uint64_t i) {
  const uint32_t n = texel_channels(f), cls = texel_class(f);
  Texel4 v = {0.0f, 0.0f, 0.0f, 1.0f};  // (no array: the channels stay in registers on the device)
  if (cls < 2) {
    const uint8_t* p = static_cast<const uint8_t*>(base) + i * n;
    v.x = decode_unorm8(p[0]);
    if (n > 1) v.y = decode_unorm8(p[1]);
    if (n > 2) v.z = decode_unorm8(p[2]);
    if (n > 3) v.w = decode_unorm8(p[3]);
    if (cls == 1) {
      v.x = srgb_to_linear(v.x);
      if (n > 1) v.y = srgb_to_linear(v.y);
      if (n > 2) v.z = srgb_to_linear(v.z);
    }
  } else if (cls == 2) {
    const uint16_t* p = static_cast<const uint16_t*>(base) + i * n;  // (the hosts and the device are little-endian)
    v.x = decode_unorm16(p[0]);
    if (n > 1) v.y = decode_unorm16(p[1]);
    if (n > 2) v.z = decode_unorm16(p[2]);
    if (n > 3) v.w = decode_unorm16(p[3]);
  } else {
    const float* p = static_cast<const float*>(base) + i * n;
    v.x = p[0];
    if (n > 1) v.y = p[1];
    if (n > 2) v.z = p[2];
    if (n > 3) v.w = p[3];
  }
  return v;
}

// Texel (x, y) of a w x h image in the canonical format f.
STHIP_CONVERT_HD inline Texel4 decode_texel(uint32_t f, const void* base, uint32_t w, uint32_t h, uint32_t x, uint32_t y) {
  (void)h;
  if (!texel_is_block(f)) return decode_linear_texel(f, base, (uint64_t)y * w + x);
  const uint64_t block = (uint64_t)(y / 4u) * ((w + 3u) / 4u) + x / 4u;
  const uint64_t* p = static_cast<const uint64_t*>(base) + block * (texel_block_bytes(f) / 8u);
  return decode_block_texel(f, p[0], texel_block_bytes(f) == 16u ? p[1] : 0ull, 4u * (y & 3u) + (x & 3u));
}

// ---- sthip_decode_texels: what post.hip hands the launch (texel_decode.hip). Device pointers. ----
struct TexelDecodeParams {
  uint32_t format;  // canonical
  uint32_t width, height;
  uint32_t dst8;      // 1: unorm8 destination, 0: binary32
  uint32_t dst_one;   // 1: one channel (`channel`), 0: RGBA
  uint32_t channel;
  const void* src;
  void* dst;
};
// Enqueues one kernel on `stream`. Alignment is the caller's (post.hip checks it).
bool texel_decode_launch(const TexelDecodeParams& p, void* stream, std::string& err);

}  // namespace sthip
