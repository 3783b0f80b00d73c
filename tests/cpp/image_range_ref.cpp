// image_range_ref.cpp — a scalar restatement of the image-range contract of include/sthip.h ("image ranges"), written from
// the header's text: per channel the minimum and maximum over the texels that are not NaN, a NaN flag per channel, a flagged
// channel is -inf / +inf, an RGBA8 byte decodes as (float)b / 255.0f (reduced as bytes, decoded once). No product code is
// included. usage: image_range_ref <in> <out>
//   in : u32 format (0 = RGBA32F, 1 = RGBA8_UNORM), u32 texel count, the texels
//   out: float lo[4], float hi[4], u32 nan_mask
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[2];
  if (std::fread(head, 4, 2, f) != 2) return 2;
  const uint32_t format = head[0], count = head[1];
  std::vector<uint8_t> payload((size_t)count * (format ? 4 : 16));
  if (!payload.empty() && std::fread(payload.data(), 1, payload.size(), f) != payload.size()) return 2;
  std::fclose(f);
  const float inf = std::numeric_limits<float>::infinity();
  float lo[4], hi[4];
  uint32_t nan_mask = 0;
  for (int c = 0; c < 4; c++) {
    if (format) {
      int b_lo = 256, b_hi = -1;
      for (uint32_t k = 0; k < count; k++) {
        const int b = payload[4 * (size_t)k + c];
        if (b < b_lo) b_lo = b;
        if (b > b_hi) b_hi = b;
      }
      lo[c] = count ? (float)b_lo / 255.0f : -inf;
      hi[c] = count ? (float)b_hi / 255.0f : inf;
      continue;
    }
    bool any = false, nan = false;
    float a = 0, b = 0;
    for (uint32_t k = 0; k < count; k++) {
      float t;
      std::memcpy(&t, payload.data() + 16 * (size_t)k + 4 * c, 4);
      if (t != t) {
        nan = true;
        continue;
      }
      if (!any || t < a) a = t;
      if (!any || t > b) b = t;
      any = true;
    }
    if (nan) nan_mask |= 1u << c;
    lo[c] = nan || !any ? -inf : a;
    hi[c] = nan || !any ? inf : b;
  }
  f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  std::fwrite(lo, 4, 4, f);
  std::fwrite(hi, 4, 4, f);
  std::fwrite(&nan_mask, 4, 1, f);
  std::fclose(f);
  return 0;
}
