// denoise.h — the filter of the denoiser (denoise.hip): what post.hip hands the passes of sthip_denoise_filter.
#pragma once

#include <stdint.h>

#include <string>

#include "../../include/sthip.h"

namespace sthip {

constexpr uint32_t DENOISE_INLINE_VIEWS = 4;  // as sthip_accumulate: a few views ride in the kernels' arguments
constexpr uint32_t DENOISE_MAX_ITERATIONS = 8;

// All pointers are device pointers. The colour images (accum_color, filter[k]) are RGBA32F or, with `half`, RGBA16F.
struct DenoiseParams {
  uint32_t width, height, view_count, instance_count;
  float history_limit, variance_boost_length, sigma_luminance_boost;
  const sthip_ViewData* views;  // device array, or null: the views travel in `inline_views`
  sthip_ViewData inline_views[DENOISE_INLINE_VIEWS];
  const sthip_VisibilityInfo* visibility;
  const sthip_DepthInfo* depth;
  const uint32_t* instance_index_map;  // may be null: identity
  void* accum_color;
  const void* accum_moments;  // float2
  void* filter[2];
  void* guide;  // float4 per pixel: {n.x, n.y, n.z, z}, written by the variance pass
};

// Enqueues estimate_variance, `iterations` filter passes and the copy_rgb of the history tap on `stream`, in that order.
// block_shape: 0 = 32x8 lanes per block, 1 = 16x16. events: null, or 20 hipEvent_t, two per slot (slot 0 = variance, 1 + i =
// pass i, 9 = copy_rgb), recorded before and after the slot's kernel; ran[slot] is set for the slots that ran.
bool denoise_launch(const DenoiseParams& p, uint32_t iterations, uint32_t filter_type, uint32_t history_tap, bool half, uint32_t block_shape, void* stream, void* const* events,
                    bool* ran, std::string& err);

}  // namespace sthip
