// material_convert.hip — glTF PBR and diffuse/specular textures to the three Disney material images, the alpha mask and its
// minimum (kernels/material_convert.hlsl: from_gltf_pbr :46-76, from_diffuse_specular :78-108, alpha_to_roughness :28-35,
// shininess_to_roughness :37-44). The arithmetic is the contract of include/sthip.h (sthip_convert_material): binary32,
// unfused, in the shader's source order; IEEE + - * / and sqrtf only. The images are linear arrays of texels.
// Memory-bound, so the 8-bit form moves 16 bytes per access: a lane takes four consecutive texels, the up to three texels
// that remain go one per lane behind them. Every other combination of formats goes one texel per lane.
#include <hip/hip_runtime.h>

#include "material_convert.h"
#include "texel_decode.h"

namespace sthip {
namespace {

constexpr uint32_t CONVERT_BLOCK = 256;
constexpr uint32_t NO_ALPHA = 0xFFFFFFFFu;  // (the largest reduced value is (1 - 2^-24) * 2^32 = 0xFFFFFF00)

struct Switches {  // upstream's specialisation constants gUseX: kernel arguments here, uniform over the launch
  bool diffuse, specular, transmittance, roughness;
  bool diffuse_srgb;  // k_material_bytes only: gDiffuse is RGBA8_SRGB, its colour bytes go through the tables
};
// The sRGB curve of a byte as k_material_bytes serves it: linear[b] = srgb_to_linear(decode_unorm8(b)), the value the generic
// kernel computes, and byte[b] = texel_quantise(linear[b]), the byte it stores for a base colour that only passes through. Each
// workgroup fills both itself, one entry per lane (CONVERT_BLOCK = 256).
struct SrgbTables {
  float linear[256];
  uint32_t byte[256];
};

__device__ __forceinline__ float luminance3(float x, float y, float z) { return (x * 0.2126f + y * 0.7152f) + z * 0.0722f; }
__device__ __forceinline__ float decode1(uint32_t b) { return decode_unorm8(b); }  // = (float)b / 255.0f
__device__ __forceinline__ float4 decode4(uint32_t w) { return make_float4(decode1(w & 0xFFu), decode1((w >> 8) & 0xFFu), decode1((w >> 16) & 0xFFu), decode1(w >> 24)); }
__device__ __forceinline__ uint32_t quantise4(float4 v) { return texel_quantise(v.x) | (texel_quantise(v.y) << 8) | (texel_quantise(v.z) << 16) | (texel_quantise(v.w) << 24); }
__device__ __forceinline__ uint32_t alpha_word(float a) { return a < 1.0f ? (uint32_t)(texel_saturate(a) * 4294967296.0f) : NO_ALPHA; }

// One texel of a material kind: decoded sources in (an absent one is ignored), the three DisneyMaterialData vectors out.
template <uint32_t KIND>
__device__ __forceinline__ void convert_texel(const Switches u, float4 d, float4 s, float4 t, float r, float4& o0, float4& o1, float4& o2) {
  if (KIND == STHIP_CONVERT_GLTF_PBR) {
    if (!u.diffuse) d = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    if (!u.specular) s = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    const float l = luminance3(d.x, d.y, d.z);
    const float transmission = u.transmittance ? texel_saturate(luminance3(t.x, t.y, t.z) / (l > 0.0f ? l : 1.0f)) : 0.0f;
    o0 = make_float4(d.x, d.y, d.z, 1.0f);
    o1 = make_float4(s.z, s.y, 1.0f, 1.0f);
    o2 = make_float4(1.0f, 1.0f, transmission, 1.0f);
  } else {
    if (!u.diffuse) d = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!u.specular) s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!u.transmittance) t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float ld = luminance3(d.x, d.y, d.z), ls = luminance3(s.x, s.y, s.z), lt = luminance3(t.x, t.y, t.z);
    const float den = (ls + ld) + lt;
    o0 = make_float4(((d.x * ld + s.x * ls) + t.x * lt) / den, ((d.y * ld + s.y * ls) + t.y * lt) / den, ((d.z * ld + s.z * ls) + t.z * lt) / den, 1.0f);
    o1 = make_float4(u.specular ? texel_saturate(ls / den) : 1.0f, u.roughness ? r : 1.0f, 1.0f, 1.0f);
    o2 = make_float4(1.0f, 1.0f, u.transmittance ? texel_saturate(lt / den) : 1.0f, 1.0f);
  }
}

// The minimum over the wave with cross-lane moves, then one vector atomic from its first lane if some lane saw a < 1.
// Every lane of the wave must arrive here. The word only ever goes down, so a wave whose minimum is not below what a plain
// device-scope load sees (a stale value is a larger one) has nothing to add and sends no atomic: without that look every wave
// of a material with some transparency queues on the one address, about 11 ns each, and the kernel runs at a ninth of the
// memory rate.
__device__ __forceinline__ void reduce_min_alpha(uint32_t v, uint32_t* min_alpha) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, off, 64));
  if ((threadIdx.x & 63u) == 0 && v != NO_ALPHA && v < __hip_atomic_load(min_alpha, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(min_alpha, v);
}

// Everything 8-bit. Lanes [0, groups) take the texels [4 lane, 4 lane + 4): one 16-byte load per present source (4 bytes of
// gRoughness), three 16-byte stores and 4 bytes of mask. Lanes [groups, groups + singles) take texel 4 groups + (lane - groups).
// A byte that only passes through (GLTF base colour, metallic, roughness; gRoughness; the mask) is copied: texel_quantise(decode1(b))
// is b for all 256 bytes, which tests/test_material_convert.py checks on the numpy statement and against the generic kernel.
// With an sRGB gDiffuse the colour bytes of the base colour become tables.byte[b] and its decoded floats tables.linear[b];
// the alpha byte is linear and passes through as before.
__device__ __forceinline__ float4 decode4_diffuse(const Switches u, const SrgbTables& tables, uint32_t w) {
  if (!u.diffuse_srgb) return decode4(w);
  return make_float4(tables.linear[w & 0xFFu], tables.linear[(w >> 8) & 0xFFu], tables.linear[(w >> 16) & 0xFFu], decode1(w >> 24));
}
template <uint32_t KIND>
__device__ __forceinline__ void bytes_texel(const Switches u, const SrgbTables& tables, uint32_t d, uint32_t s, uint32_t t, uint32_t r, uint32_t& w0, uint32_t& w1, uint32_t& w2,
                                            uint32_t& lane_min) {
  if (u.diffuse && (d >> 24) != 255u) lane_min = min(lane_min, alpha_word(decode1(d >> 24)));
  if (KIND == STHIP_CONVERT_GLTF_PBR) {
    const uint32_t base = u.diffuse_srgb ? (tables.byte[d & 0xFFu] | (tables.byte[(d >> 8) & 0xFFu] << 8) | (tables.byte[(d >> 16) & 0xFFu] << 16)) : d;
    w0 = u.diffuse ? (base | 0xFF000000u) : 0xFFFFFFFFu;
    w1 = u.specular ? (((s >> 16) & 0xFFu) | (s & 0xFF00u) | 0xFFFF0000u) : 0xFFFFFFFFu;
    uint32_t tr = 0;
    if (u.transmittance) {
      const float4 df = u.diffuse ? decode4_diffuse(u, tables, d) : make_float4(1.0f, 1.0f, 1.0f, 1.0f), tf = decode4(t);
      const float l = luminance3(df.x, df.y, df.z);
      tr = texel_quantise(texel_saturate(luminance3(tf.x, tf.y, tf.z) / (l > 0.0f ? l : 1.0f)));
    }
    w2 = 0xFF00FFFFu | (tr << 16);
  } else {
    float4 o0, o1, o2;
    convert_texel<KIND>(u, decode4_diffuse(u, tables, d), decode4(s), decode4(t), 1.0f, o0, o1, o2);
    w0 = quantise4(o0);
    w1 = (quantise4(o1) & 0xFFFF00FFu) | ((u.roughness ? r : 255u) << 8);
    w2 = quantise4(o2);
  }
}

template <uint32_t KIND>
__global__ void __launch_bounds__(CONVERT_BLOCK) k_material_bytes(Switches u, const uint32_t* __restrict__ diffuse, const uint32_t* __restrict__ specular, const uint32_t* __restrict__ transmittance,
                                                                  const uint8_t* __restrict__ roughness, uint32_t* __restrict__ out0, uint32_t* __restrict__ out1, uint32_t* __restrict__ out2,
                                                                  uint8_t* __restrict__ mask, uint32_t* __restrict__ min_alpha, uint32_t groups, uint32_t singles) {
  const uint32_t lane = blockIdx.x * CONVERT_BLOCK + threadIdx.x;
  uint32_t lane_min = NO_ALPHA;
  __shared__ SrgbTables tables;
  if (u.diffuse_srgb) {  // (uniform over the launch: every lane of the workgroup arrives at the barrier)
    const float v = srgb_to_linear(decode_unorm8(threadIdx.x));
    tables.linear[threadIdx.x] = v;
    tables.byte[threadIdx.x] = texel_quantise(v);
    __syncthreads();
  }
  if (lane < groups) {
    const uint4 zero = make_uint4(0, 0, 0, 0);
    const uint4 d = u.diffuse ? reinterpret_cast<const uint4*>(diffuse)[lane] : zero;
    const uint4 s = u.specular ? reinterpret_cast<const uint4*>(specular)[lane] : zero;
    const uint4 t = u.transmittance ? reinterpret_cast<const uint4*>(transmittance)[lane] : zero;
    const uint32_t r = u.roughness ? reinterpret_cast<const uint32_t*>(roughness)[lane] : 0u;
    uint4 w0, w1, w2;
    bytes_texel<KIND>(u, tables, d.x, s.x, t.x, r & 0xFFu, w0.x, w1.x, w2.x, lane_min);
    bytes_texel<KIND>(u, tables, d.y, s.y, t.y, (r >> 8) & 0xFFu, w0.y, w1.y, w2.y, lane_min);
    bytes_texel<KIND>(u, tables, d.z, s.z, t.z, (r >> 16) & 0xFFu, w0.z, w1.z, w2.z, lane_min);
    bytes_texel<KIND>(u, tables, d.w, s.w, t.w, r >> 24, w0.w, w1.w, w2.w, lane_min);
    reinterpret_cast<uint4*>(out0)[lane] = w0;
    reinterpret_cast<uint4*>(out1)[lane] = w1;
    reinterpret_cast<uint4*>(out2)[lane] = w2;
    if (u.diffuse) reinterpret_cast<uint32_t*>(mask)[lane] = (d.x >> 24) | ((d.y >> 24) << 8) | ((d.z >> 24) << 16) | (d.w & 0xFF000000u);
  } else if (lane - groups < singles) {
    const uint64_t i = (uint64_t)groups * 4u + (lane - groups);
    const uint32_t d = u.diffuse ? diffuse[i] : 0u, s = u.specular ? specular[i] : 0u, t = u.transmittance ? transmittance[i] : 0u;
    const uint32_t r = u.roughness ? roughness[i] : 0u;
    uint32_t w0, w1, w2;
    bytes_texel<KIND>(u, tables, d, s, t, r, w0, w1, w2, lane_min);
    out0[i] = w0;
    out1[i] = w1;
    out2[i] = w2;
    if (u.diffuse) mask[i] = (uint8_t)(d >> 24);
  }
  if (u.diffuse) reduce_min_alpha(lane_min, min_alpha);
}

// A source format is a launch-uniform byte: 0 and 1 are the library's own forms (aligned to their texel: one load), anything else a
// sthip_texel_format from 16 up, decoded by texel_decode.h at texel (i % width, i / width). A one-channel source takes channel 0.
__device__ __forceinline__ float4 load_texel4(const void* p, uint32_t format, uint32_t i, uint32_t width, uint32_t height) {
  if (format == 0) return static_cast<const float4*>(p)[i];
  if (format == 1) return decode4(static_cast<const uint32_t*>(p)[i]);
  const Texel4 v = decode_texel(format, p, width, height, i % width, i / width);
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float load_texel1(const void* p, uint32_t format, uint32_t i, uint32_t width, uint32_t height) {
  if (format == 0) return static_cast<const float*>(p)[i];
  if (format == 1) return decode1(static_cast<const uint8_t*>(p)[i]);
  return decode_texel(format, p, width, height, i % width, i / width).x;
}

// One texel per lane, any mix of source formats (uniform over the launch: `formats` holds a byte per source, gDiffuse lowest); OUT8: RGBA8 / R8 outputs, else RGBA32F / R32F.
template <uint32_t KIND, bool OUT8>
__global__ void __launch_bounds__(CONVERT_BLOCK) k_material_texels(Switches u, const void* __restrict__ diffuse, const void* __restrict__ specular, const void* __restrict__ transmittance,
                                                                   const void* __restrict__ roughness, uint32_t formats, uint32_t width, uint32_t height, void* __restrict__ out0, void* __restrict__ out1,
                                                                   void* __restrict__ out2, void* __restrict__ mask, uint32_t* __restrict__ min_alpha, uint32_t texels) {
  const uint32_t i = blockIdx.x * CONVERT_BLOCK + threadIdx.x;
  uint32_t lane_min = NO_ALPHA;
  if (i < texels) {
    const float4 none = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 d = u.diffuse ? load_texel4(diffuse, formats & 0xFFu, i, width, height) : none;
    const float4 s = u.specular ? load_texel4(specular, (formats >> 8) & 0xFFu, i, width, height) : none;
    const float4 t = u.transmittance ? load_texel4(transmittance, (formats >> 16) & 0xFFu, i, width, height) : none;
    const float r = u.roughness ? load_texel1(roughness, formats >> 24, i, width, height) : 1.0f;
    float4 o0, o1, o2;
    convert_texel<KIND>(u, d, s, t, r, o0, o1, o2);
    if (OUT8) {
      static_cast<uint32_t*>(out0)[i] = quantise4(o0);
      static_cast<uint32_t*>(out1)[i] = quantise4(o1);
      static_cast<uint32_t*>(out2)[i] = quantise4(o2);
    } else {
      static_cast<float4*>(out0)[i] = o0;
      static_cast<float4*>(out1)[i] = o1;
      static_cast<float4*>(out2)[i] = o2;
    }
    if (u.diffuse) {
      if (OUT8)
        static_cast<uint8_t*>(mask)[i] = (uint8_t)texel_quantise(d.w);
      else
        static_cast<float*>(mask)[i] = d.w;
      lane_min = alpha_word(d.w);
    }
  }
  if (u.diffuse) reduce_min_alpha(lane_min, min_alpha);
}

__device__ __forceinline__ float to_roughness(uint32_t kind, float x) {
  return kind == STHIP_CONVERT_ALPHA_TO_ROUGHNESS ? texel_saturate(sqrtf(x)) : texel_saturate(sqrtf(2.0f / (x + 2.0f)));
}

// The two roughness kinds. With 8-bit input and output, lanes [0, groups) take four texels (one 4-byte load, one 4-byte store),
// the lanes behind them one texel each; otherwise groups = 0. IN8 is false for every input that is not R8_UNORM (format 1).
template <bool IN8, bool OUT8>
__global__ void __launch_bounds__(CONVERT_BLOCK) k_to_roughness(uint32_t kind, const void* __restrict__ input, uint32_t format, uint32_t width, uint32_t height, void* __restrict__ output,
                                                                uint32_t groups, uint32_t singles) {
  const uint32_t lane = blockIdx.x * CONVERT_BLOCK + threadIdx.x;
  if (IN8 && OUT8 && lane < groups) {
    const uint32_t w = static_cast<const uint32_t*>(input)[lane];
    static_cast<uint32_t*>(output)[lane] = texel_quantise(to_roughness(kind, decode1(w & 0xFFu))) | (texel_quantise(to_roughness(kind, decode1((w >> 8) & 0xFFu))) << 8) |
                                           (texel_quantise(to_roughness(kind, decode1((w >> 16) & 0xFFu))) << 16) | (texel_quantise(to_roughness(kind, decode1(w >> 24))) << 24);
  } else if (lane >= groups && lane - groups < singles) {
    const uint64_t i = (uint64_t)groups * 4u + (lane - groups);
    const float v = to_roughness(kind, IN8 ? decode1(static_cast<const uint8_t*>(input)[i]) : load_texel1(input, format, (uint32_t)i, width, height));
    if (OUT8)
      static_cast<uint8_t*>(output)[i] = (uint8_t)texel_quantise(v);
    else
      static_cast<float*>(output)[i] = v;
  }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

bool material_convert_launch(const MaterialConvertParams& p, void* stream_, std::string& err) {
  hipStream_t stream = (hipStream_t)stream_;
  const uint32_t texels = (uint32_t)p.texels;  // (at most 2^30)
  const bool out8 = p.output_format != 0;
  auto blocks = [](uint64_t lanes) { return dim3((uint32_t)((lanes + CONVERT_BLOCK - 1) / CONVERT_BLOCK)); };
  auto finish = [&](const char* kernel) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) err = std::string(kernel) + ": " + hipGetErrorString(e);
    return e == hipSuccess;
  };
  if (p.kind == STHIP_CONVERT_ALPHA_TO_ROUGHNESS || p.kind == STHIP_CONVERT_SHININESS_TO_ROUGHNESS) {
    const bool in8 = p.input_format == 1;
    const bool four = in8 && out8 && aligned(p.input, 4) && aligned(p.roughness_rw, 4);
    const uint32_t groups = four ? texels / 4 : 0, singles = texels - groups * 4;
    const dim3 grid = blocks((uint64_t)groups + singles);
    if (in8 && out8)
      hipLaunchKernelGGL((k_to_roughness<true, true>), grid, dim3(CONVERT_BLOCK), 0, stream, p.kind, p.input, (uint32_t)p.input_format, p.width, p.height, p.roughness_rw, groups, singles);
    else if (in8)
      hipLaunchKernelGGL((k_to_roughness<true, false>), grid, dim3(CONVERT_BLOCK), 0, stream, p.kind, p.input, (uint32_t)p.input_format, p.width, p.height, p.roughness_rw, groups, singles);
    else if (out8)
      hipLaunchKernelGGL((k_to_roughness<false, true>), grid, dim3(CONVERT_BLOCK), 0, stream, p.kind, p.input, (uint32_t)p.input_format, p.width, p.height, p.roughness_rw, groups, singles);
    else
      hipLaunchKernelGGL((k_to_roughness<false, false>), grid, dim3(CONVERT_BLOCK), 0, stream, p.kind, p.input, (uint32_t)p.input_format, p.width, p.height, p.roughness_rw, groups, singles);
    return finish("k_to_roughness");
  }
  const bool gltf = p.kind == STHIP_CONVERT_GLTF_PBR;
  Switches u;
  u.diffuse = p.diffuse != nullptr;
  u.specular = p.specular != nullptr;
  u.transmittance = p.transmittance != nullptr;
  u.roughness = !gltf && p.roughness != nullptr;
  const hipError_t e = hipMemsetAsync(p.min_alpha, 0xFF, sizeof(uint32_t), stream);  // the call initialises gOutputMinAlpha
  if (e != hipSuccess) {
    err = std::string("clearing gOutputMinAlpha: ") + hipGetErrorString(e);
    return false;
  }
  // the 8-bit kernel also takes the diffuse image every glTF file has: RGBA8_SRGB, where it is aligned as an RGBA8_UNORM one is
  u.diffuse_srgb = u.diffuse && p.diffuse_format == STHIP_TEXEL_RGBA8_SRGB && aligned(p.diffuse, 4);
  const uint32_t source_bytes = (u.diffuse && (p.diffuse_format == 1 || u.diffuse_srgb) ? 1u : 0u) | (u.specular && p.specular_format == 1 ? 2u : 0u) | (u.transmittance && p.transmittance_format == 1 ? 4u : 0u) |
                                (u.roughness && p.roughness_format == 1 ? 8u : 0u);
  const uint32_t formats = (uint32_t)p.diffuse_format | ((uint32_t)p.specular_format << 8) | ((uint32_t)p.transmittance_format << 16) | ((uint32_t)p.roughness_format << 24);
  const uint32_t present = (u.diffuse ? 1u : 0u) | (u.specular ? 2u : 0u) | (u.transmittance ? 4u : 0u) | (u.roughness ? 8u : 0u);
  if (out8 && source_bytes == present) {
    const bool four = (!u.diffuse || (aligned(p.diffuse, 16) && aligned(p.alpha_mask, 4))) && (!u.specular || aligned(p.specular, 16)) && (!u.transmittance || aligned(p.transmittance, 16)) &&
                      (!u.roughness || aligned(p.roughness, 4)) && aligned(p.out[0], 16) && aligned(p.out[1], 16) && aligned(p.out[2], 16);
    const uint32_t groups = four ? texels / 4 : 0, singles = texels - groups * 4;
    const dim3 grid = blocks((uint64_t)groups + singles);
#define STHIP_BYTES_ARGS                                                                                                                                                                  \
  u, static_cast<const uint32_t*>(p.diffuse), static_cast<const uint32_t*>(p.specular), static_cast<const uint32_t*>(p.transmittance), static_cast<const uint8_t*>(p.roughness),         \
      static_cast<uint32_t*>(p.out[0]), static_cast<uint32_t*>(p.out[1]), static_cast<uint32_t*>(p.out[2]), static_cast<uint8_t*>(p.alpha_mask), p.min_alpha, groups, singles
    if (gltf)
      hipLaunchKernelGGL((k_material_bytes<STHIP_CONVERT_GLTF_PBR>), grid, dim3(CONVERT_BLOCK), 0, stream, STHIP_BYTES_ARGS);
    else
      hipLaunchKernelGGL((k_material_bytes<STHIP_CONVERT_DIFFUSE_SPECULAR>), grid, dim3(CONVERT_BLOCK), 0, stream, STHIP_BYTES_ARGS);
#undef STHIP_BYTES_ARGS
    return finish("k_material_bytes");
  }
  const dim3 grid = blocks(texels);
#define STHIP_TEXELS_ARGS u, p.diffuse, p.specular, p.transmittance, p.roughness, formats, p.width, p.height, p.out[0], p.out[1], p.out[2], p.alpha_mask, p.min_alpha, texels
  if (gltf && out8)
    hipLaunchKernelGGL((k_material_texels<STHIP_CONVERT_GLTF_PBR, true>), grid, dim3(CONVERT_BLOCK), 0, stream, STHIP_TEXELS_ARGS);
  else if (gltf)
    hipLaunchKernelGGL((k_material_texels<STHIP_CONVERT_GLTF_PBR, false>), grid, dim3(CONVERT_BLOCK), 0, stream, STHIP_TEXELS_ARGS);
  else if (out8)
    hipLaunchKernelGGL((k_material_texels<STHIP_CONVERT_DIFFUSE_SPECULAR, true>), grid, dim3(CONVERT_BLOCK), 0, stream, STHIP_TEXELS_ARGS);
  else
    hipLaunchKernelGGL((k_material_texels<STHIP_CONVERT_DIFFUSE_SPECULAR, false>), grid, dim3(CONVERT_BLOCK), 0, stream, STHIP_TEXELS_ARGS);
#undef STHIP_TEXELS_ARGS
  return finish("k_material_texels");
}

}  // namespace sthip
