// texel_decode.hip — sthip_decode_texels: a source image in an asset's own texel format (include/sthip.h: sthip_texel_format)
// to one of the library's four forms. The arithmetic is texel_decode.h, shared with the host and with the material conversion.
// Memory-bound, like material_convert.hip, so the lanes are shaped by the loads and stores:
//   block formats    a lane takes a 4 x 1 row of one block: one 8- or 16-byte load, up to four texels out, as one wide store
//                    where the row is whole and its address allows (an RGBA32F row is always four 16-byte stores);
//   linear 8-bit     lanes [0, groups) take four consecutive texels (4 * channels bytes in, one wide store out), the lanes
//                    behind them one texel each, as k_material_bytes does; sRGB bytes are served from a 256-entry table in LDS
//                    that each workgroup fills with srgb_to_linear(decode_unorm8(b)) itself, one entry per lane;
//   16-bit, binary32 one texel per lane.
#include <hip/hip_runtime.h>

#include "texel_decode.h"

namespace sthip {
namespace {

constexpr uint32_t DECODE_BLOCK = 256;  // (= the entries of the sRGB table: lane b fills entry b)

enum DecodeMode : uint32_t { MODE_BLOCK = 0, MODE_LINEAR8 = 1, MODE_LINEAR = 2 };

__device__ __forceinline__ float pick_channel(const Texel4& v, uint32_t channel) { return channel == 0 ? v.x : channel == 1 ? v.y : channel == 2 ? v.z : v.w; }
__device__ __forceinline__ uint32_t quantise_rgba(const Texel4& v) { return texel_quantise(v.x) | (texel_quantise(v.y) << 8) | (texel_quantise(v.z) << 16) | (texel_quantise(v.w) << 24); }

template <bool DST8, bool ONE>
__device__ __forceinline__ void store_one(void* dst, uint64_t i, const Texel4& v, uint32_t channel) {
  if (ONE && DST8)
    static_cast<uint8_t*>(dst)[i] = (uint8_t)texel_quantise(pick_channel(v, channel));
  else if (ONE)
    static_cast<float*>(dst)[i] = pick_channel(v, channel);
  else if (DST8)
    static_cast<uint32_t*>(dst)[i] = quantise_rgba(v);
  else
    static_cast<float4*>(dst)[i] = make_float4(v.x, v.y, v.z, v.w);
}

// Texels [i, i + 4), i a multiple of nothing in particular: the caller says whether the address takes the wide store.
template <bool DST8, bool ONE>
__device__ __forceinline__ void store_four(void* dst, uint64_t i, const Texel4& a, const Texel4& b, const Texel4& c, const Texel4& d, uint32_t channel) {
  if (ONE && DST8) {
    *reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(dst) + i) = texel_quantise(pick_channel(a, channel)) | (texel_quantise(pick_channel(b, channel)) << 8) |
                                                                   (texel_quantise(pick_channel(c, channel)) << 16) | (texel_quantise(pick_channel(d, channel)) << 24);
  } else if (ONE) {
    *reinterpret_cast<float4*>(static_cast<float*>(dst) + i) = make_float4(pick_channel(a, channel), pick_channel(b, channel), pick_channel(c, channel), pick_channel(d, channel));
  } else if (DST8) {
    *reinterpret_cast<uint4*>(static_cast<uint32_t*>(dst) + i) = make_uint4(quantise_rgba(a), quantise_rgba(b), quantise_rgba(c), quantise_rgba(d));
  } else {
    float4* o = static_cast<float4*>(dst) + i;
    o[0] = make_float4(a.x, a.y, a.z, a.w);
    o[1] = make_float4(b.x, b.y, b.z, b.w);
    o[2] = make_float4(c.x, c.y, c.z, c.w);
    o[3] = make_float4(d.x, d.y, d.z, d.w);
  }
}
// The alignment the wide store of store_four needs, in bytes, and the bytes of a destination texel.
template <bool DST8, bool ONE>
__host__ __device__ constexpr uint32_t wide_alignment() { return (ONE && DST8) ? 4u : 16u; }
template <bool DST8, bool ONE>
__host__ __device__ constexpr uint32_t dst_texel_bytes() { return ONE ? (DST8 ? 1u : 4u) : (DST8 ? 4u : 16u); }

// A texel of N 8-bit channels whose bytes start at byte j of the words w[0 .. N).
template <uint32_t N>
__device__ __forceinline__ Texel4 texel_of_bytes(const uint32_t (&w)[4], uint32_t j, bool srgb, const float* table) {
  float c[4] = {0.0f, 0.0f, 0.0f, 1.0f};
#pragma unroll
  for (uint32_t k = 0; k < N; k++) {
    const uint32_t b = (w[(j + k) >> 2] >> (8u * ((j + k) & 3u))) & 0xFFu;  // (j and k are constants after inlining and unrolling)
    c[k] = (srgb && k < 3) ? table[b] : decode_unorm8(b);
  }
  const Texel4 v = {c[0], c[1], c[2], c[3]};
  return v;
}
template <uint32_t N, bool DST8, bool ONE>
__device__ __forceinline__ void group_of_bytes(const void* src, void* dst, uint32_t lane, bool srgb, const float* table, uint32_t channel) {
  const uint32_t* p = static_cast<const uint32_t*>(src) + (uint64_t)lane * N;  // 4 texels of N bytes: N words
  uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
  for (uint32_t k = 0; k < N; k++) w[k] = p[k];
  store_four<DST8, ONE>(dst, (uint64_t)lane * 4u, texel_of_bytes<N>(w, 0, srgb, table), texel_of_bytes<N>(w, N, srgb, table), texel_of_bytes<N>(w, 2 * N, srgb, table),
                        texel_of_bytes<N>(w, 3 * N, srgb, table), channel);
}

template <uint32_t MODE, bool DST8, bool ONE>
__global__ void __launch_bounds__(DECODE_BLOCK) k_decode_texels(uint32_t f, const void* __restrict__ src, void* __restrict__ dst, uint32_t w, uint32_t h, uint32_t channel, uint32_t groups,
                                                                uint32_t lanes) {
  const uint32_t lane = blockIdx.x * DECODE_BLOCK + threadIdx.x;
  if (MODE == MODE_BLOCK) {
    // lanes = blocks_x * h: lane -> (block column, image row)
    if (lane >= lanes) return;
    const uint32_t blocks_x = (w + 3u) / 4u, bx = lane % blocks_x, y = lane / blocks_x;
    const uint64_t block = (uint64_t)(y / 4u) * blocks_x + bx;
    uint64_t lo, hi = 0;
    if (texel_block_bytes(f) == 16u) {
      const uint4 q = static_cast<const uint4*>(src)[block];
      lo = (uint64_t)q.x | ((uint64_t)q.y << 32), hi = (uint64_t)q.z | ((uint64_t)q.w << 32);
    } else {
      const uint2 q = static_cast<const uint2*>(src)[block];
      lo = (uint64_t)q.x | ((uint64_t)q.y << 32);
    }
    const uint32_t x0 = bx * 4u, count = min(4u, w - x0), t0 = 4u * (y & 3u);
    const uint64_t i = (uint64_t)y * w + x0;
    const Texel4 a = decode_block_texel(f, lo, hi, t0);
    if (count == 4u) {  // (texels beyond the extent are never decoded)
      const Texel4 b = decode_block_texel(f, lo, hi, t0 + 1u), c = decode_block_texel(f, lo, hi, t0 + 2u), d = decode_block_texel(f, lo, hi, t0 + 3u);
      const uintptr_t address = reinterpret_cast<uintptr_t>(dst) + i * dst_texel_bytes<DST8, ONE>();
      if ((!DST8 && !ONE) || (address & (wide_alignment<DST8, ONE>() - 1u)) == 0) {
        store_four<DST8, ONE>(dst, i, a, b, c, d, channel);
      } else {
        store_one<DST8, ONE>(dst, i, a, channel);
        store_one<DST8, ONE>(dst, i + 1u, b, channel);
        store_one<DST8, ONE>(dst, i + 2u, c, channel);
        store_one<DST8, ONE>(dst, i + 3u, d, channel);
      }
    } else {
      store_one<DST8, ONE>(dst, i, a, channel);
      if (count > 1u) store_one<DST8, ONE>(dst, i + 1u, decode_block_texel(f, lo, hi, t0 + 1u), channel);
      if (count > 2u) store_one<DST8, ONE>(dst, i + 2u, decode_block_texel(f, lo, hi, t0 + 2u), channel);
    }
  } else if (MODE == MODE_LINEAR8) {
    // lanes = groups + singles
    __shared__ float table[DECODE_BLOCK];
    const bool srgb = texel_is_srgb(f);
    if (srgb) {  // (uniform over the launch: every lane of the workgroup arrives at the barrier)
      table[threadIdx.x] = srgb_to_linear(decode_unorm8(threadIdx.x));
      __syncthreads();
    }
    const uint32_t n = texel_channels(f);
    if (lane < groups) {
      if (n == 1)
        group_of_bytes<1, DST8, ONE>(src, dst, lane, srgb, table, channel);
      else if (n == 2)
        group_of_bytes<2, DST8, ONE>(src, dst, lane, srgb, table, channel);
      else if (n == 3)
        group_of_bytes<3, DST8, ONE>(src, dst, lane, srgb, table, channel);
      else
        group_of_bytes<4, DST8, ONE>(src, dst, lane, srgb, table, channel);
    } else if (lane < lanes) {
      const uint64_t i = (uint64_t)groups * 4u + (lane - groups);
      const uint8_t* p = static_cast<const uint8_t*>(src) + i * n;
      Texel4 v = {0.0f, 0.0f, 0.0f, 1.0f};
      v.x = srgb ? table[p[0]] : decode_unorm8(p[0]);
      if (n > 1) v.y = srgb ? table[p[1]] : decode_unorm8(p[1]);
      if (n > 2) v.z = srgb ? table[p[2]] : decode_unorm8(p[2]);
      if (n > 3) v.w = decode_unorm8(p[3]);
      store_one<DST8, ONE>(dst, i, v, channel);
    }
  } else {
    if (lane < lanes) store_one<DST8, ONE>(dst, lane, decode_linear_texel(f, src, lane), channel);
  }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

template <uint32_t MODE>
void launch(const TexelDecodeParams& p, hipStream_t stream, uint32_t groups, uint32_t lanes) {
  const dim3 grid((lanes + DECODE_BLOCK - 1) / DECODE_BLOCK), block(DECODE_BLOCK);
  if (p.dst8 && p.dst_one)
    hipLaunchKernelGGL((k_decode_texels<MODE, true, true>), grid, block, 0, stream, p.format, p.src, p.dst, p.width, p.height, p.channel, groups, lanes);
  else if (p.dst8)
    hipLaunchKernelGGL((k_decode_texels<MODE, true, false>), grid, block, 0, stream, p.format, p.src, p.dst, p.width, p.height, p.channel, groups, lanes);
  else if (p.dst_one)
    hipLaunchKernelGGL((k_decode_texels<MODE, false, true>), grid, block, 0, stream, p.format, p.src, p.dst, p.width, p.height, p.channel, groups, lanes);
  else
    hipLaunchKernelGGL((k_decode_texels<MODE, false, false>), grid, block, 0, stream, p.format, p.src, p.dst, p.width, p.height, p.channel, groups, lanes);
}

}  // namespace

bool texel_decode_launch(const TexelDecodeParams& p, void* stream_, std::string& err) {
  hipStream_t stream = (hipStream_t)stream_;
  const uint32_t texels = p.width * p.height;  // (at most 2^30)
  if (texel_is_block(p.format)) {
    launch<MODE_BLOCK>(p, stream, 0, ((p.width + 3u) / 4u) * p.height);  // (at most the texels)
  } else if (texel_class(p.format) < 2) {
    const uint32_t wide = (p.dst8 && p.dst_one) ? 4u : 16u;
    const bool four = aligned(p.src, 4) && aligned(p.dst, wide);
    const uint32_t groups = four ? texels / 4u : 0u;
    launch<MODE_LINEAR8>(p, stream, groups, groups + (texels - groups * 4u));
  } else {
    launch<MODE_LINEAR>(p, stream, 0, texels);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) err = std::string("k_decode_texels: ") + hipGetErrorString(e);
  return e == hipSuccess;
}

}  // namespace sthip
