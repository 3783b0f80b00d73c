// image_range.h — the per-channel extremes of level 0 of an image of gImages, reduced on the device (image_range.hip):
// the scan the material analysis needs again when sthip_scene_set_images replaces texels or sthip_scene_set_material_data
// makes a record name an image for the first time. include/sthip.h states the contract ("image ranges"): minimum and maximum
// per channel over the texels that are not NaN, a NaN flag per channel, a flagged channel is -inf / +inf, infinities and
// denormals as they are; the sign of a zero result is not part of it. Plain launchers, as environment.h's.
#pragma once

#include <stdint.h>

#include <string>

namespace sthip {

constexpr uint32_t IMAGE_RANGE_PARTIAL_WORDS = 9;   // per block: 4 minima, 4 maxima (as ordered keys), the NaN bits
constexpr uint32_t IMAGE_RANGE_RESULT_WORDS = 12;   // per image: float lo[4], float hi[4], uint32 nan_mask, 3 words of padding
constexpr uint32_t IMAGE_RANGE_MAX_BLOCKS = 65535;  // "image_range_blocks"

// Blocks of k_image_range for an image of `texels` texels: `forced` (1 .. IMAGE_RANGE_MAX_BLOCKS) or, with 0, as many as the
// 16-byte units of the image fill, at most 8 per CU (2048 lanes per CU: every wave slot; the grid-stride loop takes the rest).
uint32_t image_range_blocks(uint64_t texels, bool rgba8, int cu_count, uint32_t forced);

// Two launches on `stream`: k_image_range<format> over `texels` texels at `src` (RGBA32F: 16-byte aligned, 16 bytes per
// texel; RGBA8_UNORM: 4-byte aligned, 4 bytes per texel — the kernel takes the texels before the first and behind the last
// 16-byte boundary one at a time) leaves IMAGE_RANGE_PARTIAL_WORDS words per block in `partials` (room for blocks * 9 words);
// k_image_range_fold, one wave, folds them into `result` (IMAGE_RANGE_RESULT_WORDS words). The second launch starts when the
// first has finished: the only ordering there is. texels >= 1.
bool image_range_launch(const void* src, uint64_t texels, bool rgba8, uint32_t blocks, uint32_t* partials, uint32_t* result, void* stream, std::string& err);

}  // namespace sthip
