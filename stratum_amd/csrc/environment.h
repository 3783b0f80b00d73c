// environment.h — the derived forms of an image environment, built on the device (environment.hip): the float mip chain and
// the four dist2d tables of sthip_scene_set_environment (include/sthip.h states the arithmetic; the results are the bits of
// scene_prepare.cpp layout_images and of the hosts' build_distributions). Plain launchers: device pointers, a stream, an
// error string. Launches on one stream run in order: that is the only ordering between them.
#pragma once

#include <stdint.h>

#include <string>

namespace sthip {

// k_mip_rgba32f for one level, the float twin of mip_rgba8_launch: dst (nw x nh texels, nw = max(1, w / 2), nh = max(1, h / 2))
// from src (w x h texels), both device pointers to 16-byte texels. Each channel is ((a + b) + (c + e)) * 0.25f over the source
// texels (min(2x, w - 1) | min(2x + 1, w - 1), min(2y, h - 1) | min(2y + 1, h - 1)).
bool mip_rgba32f_launch(const void* src, uint32_t w, uint32_t h, void* dst, int cu_count, void* stream, std::string& err);

// Rows a wave of k_env_rows owns (its chain lanes): the two instantiations that exist. More rows per wave fill the wave's lanes
// in the chain phase, fewer rows give more waves (a 2048-row image: 32 waves of 64 rows, 128 waves of 16): measured in
// profiles/r10/environment.json.
constexpr uint32_t ENV_ROWS_PER_WAVE_DEFAULT = 16;

struct EnvironmentTables {
  const void* texels = nullptr;   // level 0 of the image: width x height RGBA32F texels (16-byte aligned)
  uint32_t width = 0, height = 0;
  const double* sines = nullptr;  // height values s[y], from the host (libm)
  float* integrals = nullptr;     // scratch, height floats: the unnormalised integral of each row
  float* marginal_pdf = nullptr;  // [height]
  float* row_pdf = nullptr;       // [height * width]
  float* marginal_cdf = nullptr;  // [height + 1]
  float* row_cdf = nullptr;       // [height * (width + 1)]
};

// The three passes, in the order they must run on one stream:
//   k_env_rows      row_cdf[y][0] = 0 and row_cdf[y][x + 1] = the unnormalised running sum through texel x, for every x < width
//                   (so row_cdf[y][width] holds the integral until k_env_normalise sets it to 1); integrals[y] = that integral;
//                   rows_per_wave is 16 or 64
//   k_env_marginal  marginal_cdf and marginal_pdf from integrals (one block; one lane runs the chain)
//   k_env_normalise row_cdf normalised in place, row_pdf, the fallback rows, row_cdf[y][width] = 1
bool env_rows_launch(const EnvironmentTables& t, uint32_t rows_per_wave, void* stream, std::string& err);
bool env_marginal_launch(const EnvironmentTables& t, void* stream, std::string& err);
bool env_normalise_launch(const EnvironmentTables& t, void* stream, std::string& err);

}  // namespace sthip
