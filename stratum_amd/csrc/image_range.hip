// image_range.hip — see image_range.h. The minimum / maximum / NaN reduction over level 0 of an image, with the contract of
// include/sthip.h. Everything is reduced as unsigned keys whose order is the order of the values, so that no floating-point
// instruction decides a result (no flushed denormal, no quieted NaN): a byte of an RGBA8 texel is its own key (the decode
// (float)b / 255.0f is monotone and made once, at the end), a binary32 that is not a NaN maps to
//   key = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000)
// which orders -inf < ... < -0 < +0 < ... < +inf (this is where a zero's sign can differ from the host scan's: not part of the
// contract). No atomics, no flags: per-block partials with plain stores, folded by a second launch.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/sthip.h"
#include "image_range.h"

namespace sthip {
namespace {

constexpr uint32_t RANGE_BLOCK = 256;
constexpr uint32_t RANGE_WAVES = RANGE_BLOCK / 64;
constexpr uint32_t KEY_NONE_LO = 0xFFFFFFFFu, KEY_NONE_HI = 0u;  // the identities (neither is the key of a number: both map to NaN bit patterns)

__device__ inline uint32_t float_key(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ inline uint32_t key_float_bits(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

// The running values of a lane: 4 minima, 4 maxima, the NaN bits
struct Running {
  uint32_t lo[4], hi[4], nan;
};

template <uint32_t FORMAT>
__device__ inline void take_channel(Running& r, int c, uint32_t v);
template <>
__device__ inline void take_channel<STHIP_IMAGE_FORMAT_RGBA32F>(Running& r, int c, uint32_t bits) {
  const bool nan = (bits & 0x7FFFFFFFu) > 0x7F800000u;
  const uint32_t key = float_key(bits);
  r.lo[c] = min(r.lo[c], nan ? KEY_NONE_LO : key);
  r.hi[c] = max(r.hi[c], nan ? KEY_NONE_HI : key);
  r.nan |= nan ? 1u << c : 0u;
}
template <>
__device__ inline void take_channel<STHIP_IMAGE_FORMAT_RGBA8_UNORM>(Running& r, int c, uint32_t texel) {
  const uint32_t b = (texel >> (8 * c)) & 0xFFu;
  r.lo[c] = min(r.lo[c], b);
  r.hi[c] = max(r.hi[c], b);
}

// one 16-byte unit: one RGBA32F texel (a channel per word) or four RGBA8 texels (a texel per word)
template <uint32_t FORMAT>
__device__ inline void take_unit(Running& r, const uint4 u) {
  if (FORMAT == STHIP_IMAGE_FORMAT_RGBA32F) {
    take_channel<FORMAT>(r, 0, u.x);
    take_channel<FORMAT>(r, 1, u.y);
    take_channel<FORMAT>(r, 2, u.z);
    take_channel<FORMAT>(r, 3, u.w);
  } else {
#pragma unroll
    for (int c = 0; c < 4; c++) {
      take_channel<FORMAT>(r, c, u.x);
      take_channel<FORMAT>(r, c, u.y);
      take_channel<FORMAT>(r, c, u.z);
      take_channel<FORMAT>(r, c, u.w);
    }
  }
}

__device__ inline void fold_wave(Running& r) {
#pragma unroll
  for (int c = 0; c < 4; c++) {
    for (int off = 32; off > 0; off >>= 1) r.lo[c] = min(r.lo[c], (uint32_t)__shfl_xor((int)r.lo[c], off, 64));
    for (int off = 32; off > 0; off >>= 1) r.hi[c] = max(r.hi[c], (uint32_t)__shfl_xor((int)r.hi[c], off, 64));
  }
  for (int off = 32; off > 0; off >>= 1) r.nan |= (uint32_t)__shfl_xor((int)r.nan, off, 64);
}

// word k of a partial folded with another: minima, maxima, bits
__device__ inline uint32_t fold_word(uint32_t k, uint32_t a, uint32_t b) { return k < 4 ? min(a, b) : k < 8 ? max(a, b) : (a | b); }

// `units` 16-byte units at `body` in a grid-stride loop, four loads in flight per lane while four are left; with RGBA8 the
// `loose` texels that lie before the first and behind the last 16-byte boundary (at most 6: `loose_at[k]` is texel k's word
// index from `words`) go to the first lanes of block 0, one 4-byte load each. Every block writes its partial, also one that
// saw no texel (the identities).
template <uint32_t FORMAT>
__global__ void __launch_bounds__(RANGE_BLOCK) k_image_range(const uint4* __restrict__ body, uint64_t units, const uint32_t* __restrict__ words, uint64_t tail_first, uint32_t head, uint32_t loose,
                                                             uint32_t* __restrict__ partials) {
  __shared__ uint32_t wave_partial[RANGE_WAVES][IMAGE_RANGE_PARTIAL_WORDS];
  Running r;
#pragma unroll
  for (int c = 0; c < 4; c++) r.lo[c] = KEY_NONE_LO, r.hi[c] = KEY_NONE_HI;
  r.nan = 0;
  const uint64_t stride = (uint64_t)gridDim.x * RANGE_BLOCK;
  uint64_t i = (uint64_t)blockIdx.x * RANGE_BLOCK + threadIdx.x;
  for (; i + 3 * stride < units; i += 4 * stride) {
    const uint4 a = body[i], b = body[i + stride], c = body[i + 2 * stride], d = body[i + 3 * stride];
    take_unit<FORMAT>(r, a);
    take_unit<FORMAT>(r, b);
    take_unit<FORMAT>(r, c);
    take_unit<FORMAT>(r, d);
  }
  for (; i < units; i += stride) take_unit<FORMAT>(r, body[i]);
  if (FORMAT == STHIP_IMAGE_FORMAT_RGBA8_UNORM && blockIdx.x == 0 && threadIdx.x < loose) {
    const uint32_t texel = words[threadIdx.x < head ? (uint64_t)threadIdx.x : tail_first + (threadIdx.x - head)];
#pragma unroll
    for (int c = 0; c < 4; c++) take_channel<FORMAT>(r, c, texel);
  }
  fold_wave(r);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 4; c++) wave_partial[wave][c] = r.lo[c], wave_partial[wave][4 + c] = r.hi[c];
    wave_partial[wave][8] = r.nan;
  }
  __syncthreads();
  if (threadIdx.x < IMAGE_RANGE_PARTIAL_WORDS) {
    uint32_t v = wave_partial[0][threadIdx.x];
    for (uint32_t w = 1; w < RANGE_WAVES; w++) v = fold_word(threadIdx.x, v, wave_partial[w][threadIdx.x]);
    partials[(size_t)blockIdx.x * IMAGE_RANGE_PARTIAL_WORDS + threadIdx.x] = v;
  }
}

// One wave: lane l folds the partials of blocks l, l + 64, ...; the wave folds its lanes; lanes 0 .. 8 decode and store
template <uint32_t FORMAT>
__global__ void __launch_bounds__(64) k_image_range_fold(const uint32_t* __restrict__ partials, uint32_t blocks, uint32_t* __restrict__ result) {
  Running r;
#pragma unroll
  for (int c = 0; c < 4; c++) r.lo[c] = KEY_NONE_LO, r.hi[c] = KEY_NONE_HI;
  r.nan = 0;
  for (uint32_t b = threadIdx.x; b < blocks; b += 64) {
    const uint32_t* p = partials + (size_t)b * IMAGE_RANGE_PARTIAL_WORDS;
#pragma unroll
    for (int c = 0; c < 4; c++) r.lo[c] = min(r.lo[c], p[c]), r.hi[c] = max(r.hi[c], p[4 + c]);
    r.nan |= p[8];
  }
  fold_wave(r);
  if (threadIdx.x < 8) {
    const uint32_t c = threadIdx.x & 3u;
    const bool is_hi = threadIdx.x >= 4;
    uint32_t key = 0;  // (selected, not indexed: a lane-dependent index would move the running values out of registers)
#pragma unroll
    for (uint32_t k = 0; k < 4; k++)
      if (k == c) key = is_hi ? r.hi[k] : r.lo[k];
    float v;
    if ((r.nan >> c) & 1u)  // unknown: everything is possible
      v = is_hi ? __builtin_inff() : -__builtin_inff();
    else if (FORMAT == STHIP_IMAGE_FORMAT_RGBA8_UNORM)
      v = (float)key / 255.0f;
    else
      v = __uint_as_float(key_float_bits(key));
    result[threadIdx.x] = __float_as_uint(v);
  } else if (threadIdx.x == 8) {
    result[8] = r.nan;
  } else if (threadIdx.x < IMAGE_RANGE_RESULT_WORDS) {
    result[threadIdx.x] = 0u;
  }
}

}  // namespace

uint32_t image_range_blocks(uint64_t texels, bool rgba8, int cu_count, uint32_t forced) {
  if (forced) return std::min(forced, IMAGE_RANGE_MAX_BLOCKS);
  const uint64_t units = rgba8 ? (texels + 3) / 4 : texels;
  const uint64_t fill = (units + RANGE_BLOCK - 1) / RANGE_BLOCK;
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(fill, (uint64_t)std::max(1, cu_count) * 8));
}

bool image_range_launch(const void* src, uint64_t texels, bool rgba8, uint32_t blocks, uint32_t* partials, uint32_t* result, void* stream, std::string& err) {
  if (!src || !texels || !blocks || blocks > IMAGE_RANGE_MAX_BLOCKS || !partials || !result) {
    err = "image_range_launch: bad arguments";
    return false;
  }
  hipStream_t st = (hipStream_t)stream;
  if (rgba8) {
    if ((uintptr_t)src & 3u) {
      err = "image_range_launch: an RGBA8 image must be 4-byte aligned";
      return false;
    }
    const uint32_t* words = static_cast<const uint32_t*>(src);
    const uint32_t head = (uint32_t)std::min<uint64_t>(texels, ((16u - ((uintptr_t)src & 15u)) & 15u) / 4u);  // texels before the first 16-byte boundary
    const uint64_t units = (texels - head) / 4;
    const uint64_t tail_first = head + units * 4;
    const uint32_t loose = head + (uint32_t)(texels - tail_first);  // at most 3 + 3
    hipLaunchKernelGGL(k_image_range<STHIP_IMAGE_FORMAT_RGBA8_UNORM>, dim3(blocks), dim3(RANGE_BLOCK), 0, st, reinterpret_cast<const uint4*>(words + head), units, words, tail_first, head, loose, partials);
    hipLaunchKernelGGL(k_image_range_fold<STHIP_IMAGE_FORMAT_RGBA8_UNORM>, dim3(1), dim3(64), 0, st, partials, blocks, result);
  } else {
    if ((uintptr_t)src & 15u) {
      err = "image_range_launch: an RGBA32F image must be 16-byte aligned";
      return false;
    }
    hipLaunchKernelGGL(k_image_range<STHIP_IMAGE_FORMAT_RGBA32F>, dim3(blocks), dim3(RANGE_BLOCK), 0, st, static_cast<const uint4*>(src), texels, nullptr, 0ull, 0u, 0u, partials);
    hipLaunchKernelGGL(k_image_range_fold<STHIP_IMAGE_FORMAT_RGBA32F>, dim3(1), dim3(64), 0, st, partials, blocks, result);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    err = std::string("image_range_launch: ") + hipGetErrorString(e);
    return false;
  }
  return true;
}

}  // namespace sthip
