// environment.hip — see environment.h. The float mip chain and the dist2d tables of an image environment on the device, with
// the arithmetic include/sthip.h states (binary32 / binary64 as written there, no contraction: the file is compiled with
// -ffp-contract=off like the rest). Only two things are serial by contract: the x order of a row's running sum and the y order
// of the marginal's; one lane owns one such chain, everything around the chains is elementwise.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "environment.h"

namespace sthip {
namespace {

constexpr uint32_t MIP_BLOCK = 256;

__device__ inline float mip_channel(float a, float b, float c, float e) { return ((a + b) + (c + e)) * 0.25f; }

// One lane per destination texel (grid-stride). Four 16-byte loads, one 16-byte store.
__global__ void __launch_bounds__(MIP_BLOCK) k_mip_rgba32f(const float4* __restrict__ src, uint32_t w, uint32_t h, float4* __restrict__ dst, uint32_t nw, uint32_t nh) {
  const uint64_t count = (uint64_t)nw * nh;
  for (uint64_t i = (uint64_t)blockIdx.x * MIP_BLOCK + threadIdx.x; i < count; i += (uint64_t)gridDim.x * MIP_BLOCK) {
    const uint32_t y = (uint32_t)(i / nw), x = (uint32_t)(i - (uint64_t)y * nw);
    const uint32_t x0 = min(2 * x, w - 1), x1 = min(2 * x + 1, w - 1), y0 = min(2 * y, h - 1), y1 = min(2 * y + 1, h - 1);
    const float4 a = src[(uint64_t)y0 * w + x0], b = src[(uint64_t)y0 * w + x1], c = src[(uint64_t)y1 * w + x0], e = src[(uint64_t)y1 * w + x1];
    dst[i] = make_float4(mip_channel(a.x, b.x, c.x, e.x), mip_channel(a.y, b.y, c.y, e.y), mip_channel(a.z, b.z, c.z, e.z), mip_channel(a.w, b.w, c.w, e.w));
  }
}

__device__ inline float luminance(const float4 t) { return (t.x * 0.2126f + t.y * 0.7152f) + t.z * 0.0722f; }

constexpr uint32_t TILE_X = 64;      // texels of a row a wave takes per step: one per lane
constexpr uint32_t TILE_PITCH = 65;  // LDS row pitch in elements, odd so that the chain phase (lane = row, all lanes at one x) does not put
                                     // every lane on one bank: by the address arithmetic a lane's 8-byte read of f[lane][x] starts at dword
                                     // 130 lane + 2 x and its 4-byte write of sums[lane][x] at 65 lane + x. Reasoned, not measured: no
                                     // bank-conflict counter was read for this kernel

// One wave per block, R rows per wave. Per step of 64 texels: lane = x loads the texels of the R rows (a wave reads 1 KB of one
// row at a time) and leaves f(x, y) = (double)lum * s[y] in LDS; lane = row runs 64 steps of its chain out of LDS with the
// running sum in a register that is carried from step to step; lane = x stores the binary32 sums of the R rows. No atomics,
// nothing crosses waves. LDS: R * 65 * 12 bytes = 12.2 KB (R = 16) or 48.8 KB (R = 64).
template <uint32_t R>
__global__ void __launch_bounds__(64) k_env_rows(const float4* __restrict__ texels, uint32_t W, uint32_t H, const double* __restrict__ sines, float* __restrict__ row_cdf, float* __restrict__ integrals) {
  __shared__ double f[R][TILE_PITCH];
  __shared__ float sums[R][TILE_PITCH];
  const uint32_t lane = threadIdx.x, r0 = blockIdx.x * R;
  if (r0 >= H) return;
  const uint32_t rows = min(R, H - r0);
  const size_t pitch = (size_t)W + 1;
  float sum = 0.0f;  // of row r0 + lane (lanes below `rows`)
  if (lane < rows) row_cdf[(size_t)(r0 + lane) * pitch] = 0.0f;
  for (uint32_t x0 = 0; x0 < W; x0 += TILE_X) {
    const uint32_t n = min(TILE_X, W - x0);
    if (lane < n) {
#pragma unroll 4
      for (uint32_t r = 0; r < rows; r++) f[r][lane] = (double)luminance(texels[(size_t)(r0 + r) * W + x0 + lane]) * sines[r0 + r];
    }
    __syncthreads();
    if (lane < rows) {
#pragma unroll 8
      for (uint32_t x = 0; x < n; x++) {
        sum = (float)((double)sum + f[lane][x]);
        sums[lane][x] = sum;
      }
    }
    __syncthreads();  // (the next step's writes of f and of sums come after its reads here: the step's first barrier lies between)
    if (lane < n) {
#pragma unroll 4
      for (uint32_t r = 0; r < rows; r++) row_cdf[(size_t)(r0 + r) * pitch + x0 + lane + 1] = sums[r][lane];
    }
  }
  if (lane < rows) integrals[r0 + lane] = sum;
}

constexpr uint32_t MARGINAL_BLOCK = 256;
constexpr uint32_t MARGINAL_CHUNK = 4096;  // weights in LDS at a time (H may be 65 535)

// What a row weighs in the marginal: its integral, or 1 for a row that took the uniform fallback (zero, negative, NaN)
__device__ inline float row_weight(float integral) { return integral > 0 ? integral : 1.0f; }

// One block. The weights come through LDS in chunks; lane 0 runs the binary32 chain over a chunk with the carried sum in a
// register and leaves the running sums in place of the weights; the block stores them. Then the block normalises.
__global__ void __launch_bounds__(MARGINAL_BLOCK) k_env_marginal(const float* __restrict__ integrals, uint32_t H, float* marginal_cdf, float* __restrict__ marginal_pdf) {
  __shared__ float w[MARGINAL_CHUNK];
  __shared__ float total_shared;
  const uint32_t t = threadIdx.x;
  float sum = 0.0f;
  if (t == 0) marginal_cdf[0] = 0.0f;
  for (uint32_t y0 = 0; y0 < H; y0 += MARGINAL_CHUNK) {
    const uint32_t n = min(MARGINAL_CHUNK, H - y0);
    for (uint32_t j = t; j < n; j += MARGINAL_BLOCK) w[j] = row_weight(integrals[y0 + j]);
    __syncthreads();
    if (t == 0) {
#pragma unroll 8
      for (uint32_t j = 0; j < n; j++) {
        sum = sum + w[j];
        w[j] = sum;
      }
    }
    __syncthreads();
    for (uint32_t j = t; j < n; j += MARGINAL_BLOCK) marginal_cdf[y0 + j + 1] = w[j];
    __syncthreads();  // (the next chunk overwrites w)
  }
  if (t == 0) total_shared = sum;
  __threadfence_block();  // the sums other lanes stored are read below
  __syncthreads();
  const float total = total_shared;
  for (uint32_t y = t; y < H; y += MARGINAL_BLOCK) {
    if (total > 0) {
      marginal_cdf[y] = marginal_cdf[y] / total;
      marginal_pdf[y] = row_weight(integrals[y]) / total;
    } else {
      marginal_pdf[y] = 1.0f / (float)H;
      marginal_cdf[y] = (float)y / (float)H;
    }
  }
  __syncthreads();  // (entry H was stored unnormalised by some lane above)
  if (t == 0) marginal_cdf[H] = 1.0f;
}

constexpr uint32_t NORMALISE_BLOCK = 256;

// One lane per entry of row_cdf: blockIdx.y is the row, x runs over [0, W]. f is made again from the texel and s[y].
__global__ void __launch_bounds__(NORMALISE_BLOCK) k_env_normalise(const float4* __restrict__ texels, uint32_t W, const double* __restrict__ sines, const float* __restrict__ integrals, float* __restrict__ row_cdf,
                                                                   float* __restrict__ row_pdf) {
  const uint32_t x = blockIdx.x * NORMALISE_BLOCK + threadIdx.x, y = blockIdx.y;
  if (x > W) return;
  float* row = row_cdf + (size_t)y * ((size_t)W + 1);
  if (x == W) {
    row[W] = 1.0f;
    return;
  }
  const float integral = integrals[y];
  const size_t at = (size_t)y * W + x;
  if (integral > 0) {
    const double fxy = (double)luminance(texels[at]) * sines[y];
    row[x] = row[x] / integral;
    row_pdf[at] = (float)(fxy / (double)integral);
  } else {
    row_pdf[at] = 1.0f / (float)W;
    row[x] = (float)x / (float)W;
  }
}

bool launched(const char* name, std::string& err) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return true;
  err = std::string(name) + ": " + hipGetErrorString(e);
  return false;
}

bool complete(const EnvironmentTables& t, const char* name, std::string& err) {
  if (t.texels && t.width && t.height && t.width <= 0xFFFFu && t.height <= 0xFFFFu && t.sines && t.integrals && t.marginal_pdf && t.row_pdf && t.marginal_cdf && t.row_cdf) return true;
  err = std::string(name) + ": an empty image or a NULL table";
  return false;
}

}  // namespace

bool mip_rgba32f_launch(const void* src, uint32_t w, uint32_t h, void* dst, int cu_count, void* stream, std::string& err) {
  if (!src || !dst || !w || !h) {
    err = "k_mip_rgba32f: an empty level";
    return false;
  }
  const uint32_t nw = std::max(1u, w / 2), nh = std::max(1u, h / 2);
  const uint64_t count = (uint64_t)nw * nh, blocks = (count + MIP_BLOCK - 1) / MIP_BLOCK;
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)std::max(1, cu_count) * 32));
  hipLaunchKernelGGL(k_mip_rgba32f, dim3(grid), dim3(MIP_BLOCK), 0, (hipStream_t)stream, (const float4*)src, w, h, (float4*)dst, nw, nh);
  return launched("k_mip_rgba32f", err);
}

bool env_rows_launch(const EnvironmentTables& t, uint32_t rows_per_wave, void* stream, std::string& err) {
  if (!complete(t, "k_env_rows", err)) return false;
  if (rows_per_wave != 16 && rows_per_wave != 64) {
    err = "k_env_rows: rows_per_wave must be 16 or 64";
    return false;
  }
  const uint32_t grid = (t.height + rows_per_wave - 1) / rows_per_wave;
  if (rows_per_wave == 16)
    hipLaunchKernelGGL(k_env_rows<16>, dim3(grid), dim3(64), 0, (hipStream_t)stream, (const float4*)t.texels, t.width, t.height, t.sines, t.row_cdf, t.integrals);
  else
    hipLaunchKernelGGL(k_env_rows<64>, dim3(grid), dim3(64), 0, (hipStream_t)stream, (const float4*)t.texels, t.width, t.height, t.sines, t.row_cdf, t.integrals);
  return launched("k_env_rows", err);
}

bool env_marginal_launch(const EnvironmentTables& t, void* stream, std::string& err) {
  if (!complete(t, "k_env_marginal", err)) return false;
  hipLaunchKernelGGL(k_env_marginal, dim3(1), dim3(MARGINAL_BLOCK), 0, (hipStream_t)stream, t.integrals, t.height, t.marginal_cdf, t.marginal_pdf);
  return launched("k_env_marginal", err);
}

bool env_normalise_launch(const EnvironmentTables& t, void* stream, std::string& err) {
  if (!complete(t, "k_env_normalise", err)) return false;
  const dim3 grid((t.width + 1 + NORMALISE_BLOCK - 1) / NORMALISE_BLOCK, t.height);  // (height <= 65 535: the y extent of a grid)
  hipLaunchKernelGGL(k_env_normalise, grid, dim3(NORMALISE_BLOCK), 0, (hipStream_t)stream, (const float4*)t.texels, t.width, t.sines, t.integrals, t.row_cdf, t.row_pdf);
  return launched("k_env_normalise", err);
}

}  // namespace sthip
