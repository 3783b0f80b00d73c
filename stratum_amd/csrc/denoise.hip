// denoise.hip — the filter of the denoiser on the device (sthip_denoise_filter, post.hip): SVGF's variance estimate and
// the edge-stopping a-trous passes the reference dispatches after its temporal accumulation (src/Node/Denoiser.cpp:215-265):
//   k_estimate_variance  kernels/estimate_variance.hlsl:51-103
//   k_atrous             kernels/atrous.hlsl:66-262 (TapData::tap, compute_sigma_luminance, the four tap patterns, main)
//   k_copy_rgb           kernels/atrous.hlsl:266-271 (the history tap)
// The arithmetic is the contract written at sthip_denoise_desc (include/sthip.h): binary32, unfused, source order.
//
// One lane per pixel in 2-D blocks (32x8 or 16x16), so that the taps of a wave fall into few cache lines. The variance pass
// also writes the guide image {n.x, n.y, n.z, z}: a filter tap is then two 16-byte loads (colour, guide) instead of colour +
// VisibilityInfo + a strided DepthInfo and an octahedron unpack (a square root and divisions) for each of up to 24 taps. The
// guide holds exactly the values the shader's tap would have computed, so results do not depend on it. Every lane writes only
// its own pixel; a pass reads one image and writes the other, and the kernel boundary orders the passes: no atomics, no LDS.
// k_atrous is instantiated per tap pattern with the taps unrolled and the weights folded; the two "then subsampled" filter
// types pick their pattern per pass on the host.
#include <hip/hip_runtime.h>

#include <string>

#include "denoise.h"
#include "device_math.h"
#include "media.h"  // (shading.h names its types)
#include "shading.h"

namespace sthip {
namespace {

enum TapPattern { PATTERN_ATROUS, PATTERN_BOX3, PATTERN_BOX5, PATTERN_SUBSAMPLED };

DEV bool inside_view(const sthip_ViewData& v, int x, int y) { return x >= v.image_min[0] && y >= v.image_min[1] && x < v.image_max[0] && y < v.image_max[1]; }
DEV int view_of(const sthip_ViewData* views, uint32_t view_count, int x, int y) {
  for (uint32_t v = 0; v < view_count; v++)
    if (inside_view(views[v], x, y)) return (int)v;
  return -1;
}
DEV float max_k(float a, float k) { return a > k ? a : k; }  // max(a, K): a NaN gives K
DEV float squarings(float d, int n) {
#pragma unroll
  for (int k = 0; k < n; k++) d = d * d;
  return d;
}

template <typename C>
__global__ void __launch_bounds__(256) k_estimate_variance(const DenoiseParams p) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= p.width || y >= p.height) return;
  const sthip_ViewData* views = p.views ? p.views : p.inline_views;
  const int view_index = view_of(views, p.view_count, (int)x, (int)y);
  if (view_index < 0) return;
  const sthip_ViewData& view = views[view_index];
  const size_t i = (size_t)y * p.width + x;
  const C* accum = static_cast<const C*>(p.accum_color);
  const float2* moments = static_cast<const float2*>(p.accum_moments);
  float4 c = load_px(accum, i);
  float2 m = moments[i];
  const sthip_VisibilityInfo vis = p.visibility[i];
  const sthip_DepthInfo depth = p.depth[i];
  const f3 nc = unpack_normal_octahedron(vis.packed_normal);
  static_cast<float4*>(p.guide)[i] = make_float4(nc.x, nc.y, nc.z, depth.z);
  C* out = static_cast<C*>(p.filter[0]);
  const uint32_t inst = vis.instance_primitive_index & 0xFFFFu;
  if (inst == STHIP_INVALID_INSTANCE || c.w >= p.history_limit) {
    store_px(out, i, make_float4(c.x, c.y, c.z, fabsf(m.y - m.x * m.x)));
    return;
  }
  const uint32_t mapped = p.instance_index_map ? (inst < p.instance_count ? p.instance_index_map[inst] : 0xFFFFFFFFu) : inst;
  float sum_w = 1;
  const int r = c.w > 1 ? 2 : 3;
  for (int yy = -r; yy <= r; yy++)
    for (int xx = -r; xx <= r; xx++) {
      if (xx == 0 && yy == 0) continue;
      const int px = (int)x + xx, py = (int)y + yy;
      if (!inside_view(view, px, py)) continue;
      const size_t q = (size_t)py * p.width + px;
      const sthip_VisibilityInfo vp = p.visibility[q];
      if (mapped != (vp.instance_primitive_index & 0xFFFFu)) continue;
      const float fx = depth.dz_dxy[0] * (float)xx, fy = depth.dz_dxy[1] * (float)yy;
      const float w_z = fabsf(p.depth[q].z - depth.z) / (sqrtf(fx * fx + fy * fy) + 1e-2f);
      const float d = dot3(unpack_normal_octahedron(vp.packed_normal), nc);
      const float w_n = squarings(d > 0 ? (d < 1 ? d : 1.0f) : 0.0f, 7);
      const float a = -w_z;
      if (a != a || a < -87.0f) continue;
      const float w = det_expf(a) * w_n;
      if (w != w || isinf(w)) continue;
      const float2 mp = moments[q];
      m.x += mp.x * w;
      m.y += mp.y * w;
      const float4 cp = load_px(accum, q);
      c.x += cp.x * w;
      c.y += cp.y * w;
      c.z += cp.z * w;
      sum_w += w;
    }
  sum_w = 1 / sum_w;
  m.x *= sum_w;
  m.y *= sum_w;
  c.x *= sum_w;
  c.y *= sum_w;
  c.z *= sum_w;
  float v = fabsf(m.y - m.x * m.x);
  if (p.variance_boost_length > 0) v *= max_k(p.variance_boost_length / (1 + c.w), 1.0f);
  store_px(out, i, make_float4(c.x, c.y, c.z, v));
}

// TapData of atrous.hlsl: what a pixel carries from tap to tap
template <typename C>
struct Taps {
  const C* input;
  const float4* guide;
  const sthip_ViewData* view;
  uint32_t width;
  int x, y, step;
  f3 center_normal;
  float z_center, dzx, dzy, l_center, sigma_l;
  float4 sum_color;
  float sum_weight;

  // (kx, ky): the pattern's offset in taps; tap() of the shader receives it multiplied by the step
  DEV void tap(int kx, int ky, float kernel_weight) {
    const int ox = kx * step, oy = ky * step;
    const int px = x + ox, py = y + oy;
    if (!inside_view(*view, px, py)) return;
    const size_t q = (size_t)py * width + px;
    const float4 color_p = load_px(input, q);
    const float4 g = guide[q];
    const float l_p = luminance3(xyz(color_p));
    const float w_l = fabsf(l_p - l_center) / max_k(sigma_l, 1e-10f);
    const float fx = dzx * (float)(ox * step), fy = dzy * (float)(oy * step);  // the offset times the step once more, signed
    const float w_z = fabsf(g.w - z_center) / (sqrtf(fx * fx + fy * fy) + 1e-2f);
    const float w_n = squarings(max_k(dot3(xyz(g), center_normal), 0.0f), 8);
    const float a = -(w_l * w_l) - w_z;
    if (a != a || a < -87.0f) return;
    const float w = det_expf(a) * kernel_weight * w_n;
    if (w != w || isinf(w)) return;
    sum_color.x += color_p.x * w;
    sum_color.y += color_p.y * w;
    sum_color.z += color_p.z * w;
    sum_color.w += color_p.w * (w * w);
    sum_weight += w;
  }
};

template <typename C, int PATTERN>
__global__ void __launch_bounds__(256) k_atrous(const DenoiseParams p, const uint32_t iteration, const int step) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= p.width || y >= p.height) return;
  const sthip_ViewData* views = p.views ? p.views : p.inline_views;
  const int view_index = view_of(views, p.view_count, (int)x, (int)y);
  if (view_index < 0) return;
  const size_t i = (size_t)y * p.width + x;
  Taps<C> t;
  t.input = static_cast<const C*>(p.filter[iteration & 1u]);
  t.guide = static_cast<const float4*>(p.guide);
  t.view = &views[view_index];
  t.width = p.width;
  t.x = (int)x;
  t.y = (int)y;
  t.step = step;
  const float4 g = t.guide[i];
  const sthip_DepthInfo depth = p.depth[i];
  t.center_normal = xyz(g);
  t.z_center = g.w;
  t.dzx = depth.dz_dxy[0];
  t.dzy = depth.dz_dxy[1];
  t.sum_weight = 1;
  t.sum_color = load_px(t.input, i);
  t.l_center = luminance3(xyz(t.sum_color));

  {  // compute_sigma_luminance, atrous.hlsl:82-96: kernel[|xx|][|yy|] of {{1/4, 1/8}, {1/8, 1/16}}, the centre with [1][1]
    float s = t.sum_color.w * 0.0625f;
#pragma unroll
    for (int yy = -1; yy <= 1; yy++)
#pragma unroll
      for (int xx = -1; xx <= 1; xx++) {
        if (xx == 0 && yy == 0) continue;
        const int px = t.x + xx, py = t.y + yy;
        if (!inside_view(*t.view, px, py)) continue;
        s += load_px(t.input, (size_t)py * p.width + px).w * ((xx != 0 && yy != 0) ? 0.0625f : 0.125f);
      }
    t.sigma_l = sqrtf(max_k(s, 0.0f)) * p.sigma_luminance_boost;
  }

  if (!isinf(t.z_center)) {  // only foreground pixels are filtered
    if (PATTERN == PATTERN_ATROUS) {
      t.tap(1, 0, 2.0f / 3.0f);
      t.tap(0, 1, 2.0f / 3.0f);
      t.tap(-1, 0, 2.0f / 3.0f);
      t.tap(0, -1, 2.0f / 3.0f);

      t.tap(2, 0, 1.0f / 6.0f);
      t.tap(0, 2, 1.0f / 6.0f);
      t.tap(-2, 0, 1.0f / 6.0f);
      t.tap(0, -2, 1.0f / 6.0f);

      t.tap(1, 1, 4.0f / 9.0f);
      t.tap(-1, 1, 4.0f / 9.0f);
      t.tap(-1, -1, 4.0f / 9.0f);
      t.tap(1, -1, 4.0f / 9.0f);

      t.tap(1, 2, 1.0f / 9.0f);
      t.tap(-1, 2, 1.0f / 9.0f);
      t.tap(-1, -2, 1.0f / 9.0f);
      t.tap(1, -2, 1.0f / 9.0f);

      t.tap(2, 1, 1.0f / 9.0f);
      t.tap(-2, 1, 1.0f / 9.0f);
      t.tap(-2, -1, 1.0f / 9.0f);
      t.tap(2, -1, 1.0f / 9.0f);

      t.tap(2, 2, 1.0f / 36.0f);
      t.tap(-2, 2, 1.0f / 36.0f);
      t.tap(-2, -2, 1.0f / 36.0f);
      t.tap(2, -2, 1.0f / 36.0f);
    } else if (PATTERN == PATTERN_BOX3 || PATTERN == PATTERN_BOX5) {
      constexpr int r = PATTERN == PATTERN_BOX3 ? 1 : 2;
#pragma unroll
      for (int yy = -r; yy <= r; yy++)
#pragma unroll
        for (int xx = -r; xx <= r; xx++)
          if (xx != 0 || yy != 0) t.tap(xx, yy, 1.0f);
    } else {  // subsampled, atrous.hlsl:121-157
      if ((iteration & 1u) == 0) {
        t.tap(-2, 0, 1.0f);
        t.tap(2, 0, 1.0f);
      } else {
        t.tap(0, -2, 1.0f);
        t.tap(0, 2, 1.0f);
      }
      t.tap(-1, 1, 1.0f);
      t.tap(1, 1, 1.0f);
      t.tap(-1, -1, 1.0f);
      t.tap(1, -1, 1.0f);
    }
  }

  const float inv_w = 1 / t.sum_weight;
  store_px(static_cast<C*>(p.filter[(iteration + 1u) & 1u]), i,
           make_float4(t.sum_color.x * inv_w, t.sum_color.y * inv_w, t.sum_color.z * inv_w, t.sum_color.w * (inv_w * inv_w)));
}

template <typename C>
__global__ void __launch_bounds__(256) k_copy_rgb(const C* filter0, C* accum, uint32_t width, uint32_t height) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= width || y >= height) return;
  const size_t i = (size_t)y * width + x;
  const float4 f = load_px(filter0, i);
  store_px(accum, i, make_float4(f.x, f.y, f.z, load_px(accum, i).w));
}

template <typename C>
void launch_atrous(int pattern, dim3 grid, dim3 block, hipStream_t st, const DenoiseParams& p, uint32_t iteration) {
  const int step = 1 << iteration;
  switch (pattern) {
    case PATTERN_ATROUS: hipLaunchKernelGGL((k_atrous<C, PATTERN_ATROUS>), grid, block, 0, st, p, iteration, step); break;
    case PATTERN_BOX3: hipLaunchKernelGGL((k_atrous<C, PATTERN_BOX3>), grid, block, 0, st, p, iteration, step); break;
    case PATTERN_BOX5: hipLaunchKernelGGL((k_atrous<C, PATTERN_BOX5>), grid, block, 0, st, p, iteration, step); break;
    default: hipLaunchKernelGGL((k_atrous<C, PATTERN_SUBSAMPLED>), grid, block, 0, st, p, iteration, step); break;
  }
}

// the switch of atrous.hlsl:231-257: the pattern pass `iteration` (step 1 << iteration) takes
int pattern_of(uint32_t filter_type, uint32_t iteration) {
  switch (filter_type) {
    case STHIP_FILTER_BOX3: return PATTERN_BOX3;
    case STHIP_FILTER_BOX5: return PATTERN_BOX5;
    case STHIP_FILTER_SUBSAMPLED: return PATTERN_SUBSAMPLED;
    case STHIP_FILTER_BOX3_SUBSAMPLED: return iteration == 0 ? PATTERN_BOX3 : PATTERN_SUBSAMPLED;
    case STHIP_FILTER_BOX5_SUBSAMPLED: return iteration == 0 ? PATTERN_BOX5 : PATTERN_SUBSAMPLED;
    default: return PATTERN_ATROUS;
  }
}

template <typename C>
hipError_t launch_all(const DenoiseParams& p, uint32_t iterations, uint32_t filter_type, uint32_t history_tap, uint32_t block_shape, hipStream_t st, hipEvent_t* ev, bool* ran) {
  const dim3 block = block_shape == 1 ? dim3(16, 16) : dim3(32, 8);
  const dim3 grid((p.width + block.x - 1) / block.x, (p.height + block.y - 1) / block.y);
  hipError_t e = hipSuccess;
  auto bracket = [&](int slot, bool after) {
    if (!ev || e != hipSuccess) return;
    e = hipEventRecord(ev[2 * slot + (after ? 1 : 0)], st);
    if (after && ran) ran[slot] = true;
  };
  bracket(0, false);
  hipLaunchKernelGGL(k_estimate_variance<C>, grid, block, 0, st, p);
  bracket(0, true);
  for (uint32_t i = 0; i < iterations; i++) {
    bracket(1 + (int)i, false);
    launch_atrous<C>(pattern_of(filter_type, i), grid, block, st, p, i);
    bracket(1 + (int)i, true);
    if (i + 1 == history_tap) {
      bracket(9, false);
      hipLaunchKernelGGL(k_copy_rgb<C>, grid, block, 0, st, static_cast<const C*>(p.filter[0]), static_cast<C*>(p.accum_color), p.width, p.height);
      bracket(9, true);
    }
  }
  const hipError_t le = hipGetLastError();
  return e != hipSuccess ? e : le;
}

}  // namespace

bool denoise_launch(const DenoiseParams& p, uint32_t iterations, uint32_t filter_type, uint32_t history_tap, bool half, uint32_t block_shape, void* stream, void* const* events,
                    bool* ran, std::string& err) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipEvent_t* ev = reinterpret_cast<hipEvent_t*>(const_cast<void**>(events));
  const hipError_t e = half ? launch_all<Half4>(p, iterations, filter_type, history_tap, block_shape, st, ev, ran) : launch_all<float4>(p, iterations, filter_type, history_tap, block_shape, st, ev, ran);
  if (e != hipSuccess) {
    err = std::string("denoise: ") + hipGetErrorString(e);
    return false;
  }
  return true;
}

}  // namespace sthip
