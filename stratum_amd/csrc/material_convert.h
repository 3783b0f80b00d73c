// material_convert.h — the four conversions of sthip_convert_material (material_convert.hip): what post.hip hands the launch.
#pragma once

#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/sthip.h"

#ifdef __HIPCC__
#define STHIP_CONVERT_HD __host__ __device__
#else
#define STHIP_CONVERT_HD
#endif

namespace sthip {

// The decode of a byte, (float)b / 255.0f correctly rounded, without the division (eleven instructions on the device, and a
// material kernel decodes up to ten channels per texel): the product with RN(1 / 255), then one Newton step on its residual,
// both as explicit fused operations. For b = 0 .. 255 the result IS the IEEE quotient, bit for bit — all 256 are compared with
// the division by tests/cpp/material_convert_decode_check.cpp, on the host, and by the GPU tests through every kernel.
STHIP_CONVERT_HD inline float decode_unorm8(uint32_t b) {
  const float f = (float)b, k = 1.0f / 255.0f;
  const float q = f * k;
  return fmaf(fmaf(-q, 255.0f, f), k, q);
}

// All pointers are device pointers; a null source is upstream's gUseX = false. A format is 0 or 1 (sthip_image_format, 1 = bytes)
// or a sthip_texel_format from 16 up, which the generic kernels decode with texel_decode.h.
struct MaterialConvertParams {
  uint32_t kind;    // STHIP_CONVERT_*
  uint64_t texels;  // width * height, 1 .. 2^30
  uint32_t width, height;
  const void* diffuse;
  const void* specular;
  const void* transmittance;
  const void* roughness;  // one channel, DIFFUSE_SPECULAR only
  const void* input;      // one channel, the roughness kinds only
  uint8_t diffuse_format, specular_format, transmittance_format, roughness_format, input_format;
  uint32_t output_format;  // 1: RGBA8 / R8, 0: RGBA32F / R32F
  void* out[3];
  void* alpha_mask;     // one channel, written when `diffuse` is given
  uint32_t* min_alpha;  // one word, set to 0xFFFFFFFF on the stream before the kernel
  void* roughness_rw;   // one channel, the roughness kinds only
};

// Enqueues the clear of min_alpha (material kinds) and one kernel on `stream`. Alignment is the caller's (post.hip checks it):
// 4 bytes for an RGBA8 image, 16 for RGBA32F, 4 for R32F. Images that are all 8-bit and 16-byte aligned (one-channel ones 4)
// go four texels per lane.
bool material_convert_launch(const MaterialConvertParams& p, void* stream, std::string& err);

}  // namespace sthip
