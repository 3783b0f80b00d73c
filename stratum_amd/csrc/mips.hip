// mips.hip — the mip chain of an RGBA8 image on the device (include/sthip.h: STHIP_IMAGE_FORMAT_RGBA8_UNORM). Only level 0
// crosses the host link; every further level is one launch of k_mip_rgba8 over the level before it, in stream order.
// Integer arithmetic: a level is exactly what the numpy statement in tests/test_image_formats.py gives.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mips.h"

namespace sthip {
namespace {

constexpr uint32_t MIP_BLOCK = 256;

// One lane per destination texel (grid-stride). Four 4-byte loads, one 4-byte store. The even and the odd bytes of the four
// words are summed in two 16-bit lanes each (4 x 255 + 2 < 2^16: no carry crosses a lane), so a texel is two adds per word.
__global__ void __launch_bounds__(MIP_BLOCK) k_mip_rgba8(const uint32_t* __restrict__ src, uint32_t w, uint32_t h, uint32_t* __restrict__ dst, uint32_t nw, uint32_t nh) {
  const uint64_t count = (uint64_t)nw * nh;
  for (uint64_t i = (uint64_t)blockIdx.x * MIP_BLOCK + threadIdx.x; i < count; i += (uint64_t)gridDim.x * MIP_BLOCK) {
    const uint32_t y = (uint32_t)(i / nw), x = (uint32_t)(i - (uint64_t)y * nw);
    const uint32_t x0 = min(2 * x, w - 1), x1 = min(2 * x + 1, w - 1), y0 = min(2 * y, h - 1), y1 = min(2 * y + 1, h - 1);
    const uint32_t a = src[(uint64_t)y0 * w + x0], b = src[(uint64_t)y0 * w + x1], c = src[(uint64_t)y1 * w + x0], d = src[(uint64_t)y1 * w + x1];
    const uint32_t even = (a & 0x00FF00FFu) + (b & 0x00FF00FFu) + (c & 0x00FF00FFu) + (d & 0x00FF00FFu) + 0x00020002u;
    const uint32_t odd = ((a >> 8) & 0x00FF00FFu) + ((b >> 8) & 0x00FF00FFu) + ((c >> 8) & 0x00FF00FFu) + ((d >> 8) & 0x00FF00FFu) + 0x00020002u;
    dst[i] = ((even >> 2) & 0x00FF00FFu) | (((odd >> 2) & 0x00FF00FFu) << 8);
  }
}

}  // namespace

bool mip_rgba8_launch(const uint32_t* src, uint32_t w, uint32_t h, uint32_t* dst, int cu_count, void* stream, std::string& err) {
  if (!src || !dst || !w || !h) {
    err = "k_mip_rgba8: an empty level";
    return false;
  }
  const uint32_t nw = std::max(1u, w / 2), nh = std::max(1u, h / 2);
  const uint64_t count = (uint64_t)nw * nh, blocks = (count + MIP_BLOCK - 1) / MIP_BLOCK;
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)std::max(1, cu_count) * 32));
  hipLaunchKernelGGL(k_mip_rgba8, dim3(grid), dim3(MIP_BLOCK), 0, (hipStream_t)stream, src, w, h, dst, nw, nh);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    err = std::string("k_mip_rgba8: ") + hipGetErrorString(e);
    return false;
  }
  return true;
}

}  // namespace sthip
