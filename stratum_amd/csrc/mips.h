// mips.h — the mip chain of an 8-bit image, built on the device (mips.hip): what api.hip hands the kernel of
// sthip_scene_upload_formats for every level above 0 of an RGBA8 image.
#pragma once

#include <stdint.h>

#include <string>

namespace sthip {

// Enqueues k_mip_rgba8 for one level: dst (nw x nh texels, nw = max(1, w / 2), nh = max(1, h / 2)) from src (w x h texels),
// both device pointers to one 32-bit word per texel (R in the low byte). Each channel of a destination texel is
// (a + b + c + d + 2) >> 2 over the source texels (min(2x, w - 1) | min(2x + 1, w - 1), min(2y, h - 1) | min(2y + 1, h - 1)).
// Launches on one stream run in order: that is what orders level k + 1 behind level k.
bool mip_rgba8_launch(const uint32_t* src, uint32_t w, uint32_t h, uint32_t* dst, int cu_count, void* stream, std::string& err);

}  // namespace sthip
