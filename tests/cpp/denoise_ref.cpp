// denoise_ref — the reference of tests/test_denoise.py: a scalar, per-pixel restatement of the three shaders the
// denoiser's filter dispatches (kernels/estimate_variance.hlsl, kernels/atrous.hlsl: main and copy_rgb; host loop
// src/Node/Denoiser.cpp:215-265) under the arithmetic contract written at sthip_denoise_desc (include/sthip.h). It reads the
// bindings the shaders read (gVisibility, gDepth per tap: no guide image) and is built with g++ -O2 -ffp-contract=off.
//
// usage: denoise_ref <in> <out> [--half]
//   in : 12 x 4 bytes   "DNR1", width, height, view_count, instance_count (0: no gInstanceIndexMap), iterations,
//                       filter_type, history_tap, history_limit, variance_boost_length, sigma_luminance_boost (f32), 0
//        then gViews (48 B each), gVisibility (8 B per pixel), gDepth (16 B), gInstanceIndexMap (4 B per instance),
//        gAccumColor (RGBA32F), gAccumMoments (RG32F), gFilterImages[0], gFilterImages[1] (RGBA32F: what they hold before)
//   out: gFilterImages[0], gFilterImages[1], gAccumColor as RGBA32F; with --half as RGBA16F (4 x uint16 per pixel)
// --half: the colour images are RGBA16F. The inputs must hold half-representable values; every pass rounds its one store
// with det_f32tof16 and the next reads that half exactly.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "../../include/sthip_detmath.h"
#include "../../include/sthip_wire.h"

struct Float4 {
  float x, y, z, w;
};
struct Float2 {
  float x, y;
};
struct Float3 {
  float x, y, z;
};

static bool g_half = false;
static float round_store(float v) { return g_half ? det_f16tof32(det_f32tof16(v)) : v; }
static void store(std::vector<Float4>& img, size_t i, Float4 v) { img[i] = Float4{round_store(v.x), round_store(v.y), round_store(v.z), round_store(v.w)}; }

static float luminance(Float4 c) { return c.x * 0.2126f + c.y * 0.7152f + c.z * 0.0722f; }
static float dot(Float3 a, Float3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
// bitfield.h:66-75 (unpack_normal_octahedron), normalize = one division, three multiplies
static Float3 normal_of(const sthip_VisibilityInfo& v) {
  const float px = det_f16tof32(v.packed_normal & 0xFFFFu), py = det_f16tof32(v.packed_normal >> 16);
  Float3 n{px, py, 1.0f - (fabsf(px) + fabsf(py))};
  if (n.z < 0) {
    const float qx = (1.0f - fabsf(n.y)) * (n.x >= 0 ? 1.0f : -1.0f);
    const float qy = (1.0f - fabsf(n.x)) * (n.y >= 0 ? 1.0f : -1.0f);
    n.x = qx;
    n.y = qy;
  }
  const float inv = 1.0f / sqrtf(dot(n, n));
  return Float3{n.x * inv, n.y * inv, n.z * inv};
}
static uint32_t instance_of(const sthip_VisibilityInfo& v) { return v.instance_primitive_index & 0xFFFFu; }
static float length2(float x, float y) { return sqrtf(x * x + y * y); }
static float repeated_square(float d, int n) {
  for (int k = 0; k < n; k++) d = d * d;
  return d;
}

struct Problem {
  uint32_t width, height, view_count, instance_count, iterations, filter_type, history_tap;
  float history_limit, variance_boost_length, sigma_luminance_boost;
  std::vector<sthip_ViewData> views;
  std::vector<sthip_VisibilityInfo> visibility;
  std::vector<sthip_DepthInfo> depth;
  std::vector<uint32_t> instance_index_map;
  std::vector<Float4> accum_color;
  std::vector<Float2> accum_moments;
  std::vector<Float4> filter[2];

  bool inside(uint32_t view, int x, int y) const {
    const sthip_ViewData& v = views[view];
    return x >= v.image_min[0] && y >= v.image_min[1] && x < v.image_max[0] && y < v.image_max[1];
  }
  int view_of(int x, int y) const {
    for (uint32_t v = 0; v < view_count; v++)
      if (inside(v, x, y)) return (int)v;
    return -1;
  }
  size_t at(int x, int y) const { return (size_t)y * width + (size_t)x; }
};

// estimate_variance.hlsl:51-103
static void estimate_variance(Problem& P, int x, int y) {
  const int view = P.view_of(x, y);
  if (view == -1) return;
  const size_t i = P.at(x, y);
  Float4 c = P.accum_color[i];
  Float2 m = P.accum_moments[i];
  const sthip_VisibilityInfo vis = P.visibility[i];
  const float histlen = c.w;
  if (instance_of(vis) == STHIP_INVALID_INSTANCE || histlen >= P.history_limit) {
    store(P.filter[0], i, Float4{c.x, c.y, c.z, fabsf(m.y - m.x * m.x)});
    return;
  }
  const sthip_DepthInfo depth = P.depth[i];
  const Float3 n_center = normal_of(vis);
  uint32_t mapped = instance_of(vis);
  if (!P.instance_index_map.empty()) mapped = mapped < P.instance_count ? P.instance_index_map[mapped] : 0xFFFFFFFFu;
  float sum_w = 1;
  const int r = histlen > 1 ? 2 : 3;
  for (int yy = -r; yy <= r; yy++)
    for (int xx = -r; xx <= r; xx++) {
      if (xx == 0 && yy == 0) continue;
      const int px = x + xx, py = y + yy;
      if (!P.inside((uint32_t)view, px, py)) continue;
      const size_t q = P.at(px, py);
      const sthip_VisibilityInfo vis_p = P.visibility[q];
      if (mapped != instance_of(vis_p)) continue;
      const float w_z = fabsf(P.depth[q].z - depth.z) / (length2(depth.dz_dxy[0] * (float)xx, depth.dz_dxy[1] * (float)yy) + 1e-2f);
      float d = dot(normal_of(vis_p), n_center);
      d = d > 0 ? (d < 1 ? d : 1.0f) : 0.0f;  // saturate
      const float w_n = repeated_square(d, 7);  // pow(., 128)
      const float a = -w_z;
      if (a != a) continue;
      if (a < -87.0f) continue;  // w = 0: adds nothing
      const float w = det_expf(a) * w_n;
      if (std::isnan(w) || std::isinf(w)) continue;
      m.x += P.accum_moments[q].x * w;
      m.y += P.accum_moments[q].y * w;
      c.x += P.accum_color[q].x * w;
      c.y += P.accum_color[q].y * w;
      c.z += P.accum_color[q].z * w;
      sum_w += w;
    }
  sum_w = 1 / sum_w;
  m.x *= sum_w;
  m.y *= sum_w;
  c.x *= sum_w;
  c.y *= sum_w;
  c.z *= sum_w;
  float v = fabsf(m.y - m.x * m.x);
  if (P.variance_boost_length > 0) {
    const float b = P.variance_boost_length / (1 + c.w);
    v *= b > 1.0f ? b : 1.0f;
  }
  store(P.filter[0], i, Float4{c.x, c.y, c.z, v});
}

// atrous.hlsl:66-118
struct TapData {
  const Problem* P;
  const std::vector<Float4>* input;
  uint32_t view_index;
  int ix, iy;
  int step_size;
  Float3 center_normal;
  float z_center, dz_center[2], l_center, sigma_l;
  Float4 sum_color;
  float sum_weight;

  void compute_sigma_luminance() {
    const float kernel[2][2] = {{1.0f / 4.0f, 1.0f / 8.0f}, {1.0f / 8.0f, 1.0f / 16.0f}};
    float s = sum_color.w * kernel[1][1];
    for (int yy = -1; yy <= 1; yy++)
      for (int xx = -1; xx <= 1; xx++) {
        if (xx == 0 && yy == 0) continue;
        const int px = ix + xx, py = iy + yy;
        if (!P->inside(view_index, px, py)) continue;
        s += (*input)[P->at(px, py)].w * kernel[xx < 0 ? -xx : xx][yy < 0 ? -yy : yy];
      }
    sigma_l = sqrtf(s > 0.0f ? s : 0.0f) * P->sigma_luminance_boost;
  }
  // (ox, oy): the offset as main's callers pass it, already multiplied by the step
  void tap(int ox, int oy, float kernel_weight) {
    const int px = ix + ox, py = iy + oy;
    if (!P->inside(view_index, px, py)) return;
    const size_t q = P->at(px, py);
    const Float4 color_p = (*input)[q];
    const float l_p = luminance(color_p);
    const float w_l = fabsf(l_p - l_center) / (sigma_l > 1e-10f ? sigma_l : 1e-10f);
    const sthip_VisibilityInfo vis_p = P->visibility[q];
    const sthip_DepthInfo depth_p = P->depth[q];
    const int32_t sx = ox * step_size, sy = oy * step_size;  // offset * gStepSize again, signed
    const float w_z = fabsf(depth_p.z - z_center) / (length2(dz_center[0] * (float)sx, dz_center[1] * (float)sy) + 1e-2f);
    const float d = dot(normal_of(vis_p), center_normal);
    const float w_n = repeated_square(d > 0.0f ? d : 0.0f, 8);  // pow(max(0, .), 256)
    const float a = -(w_l * w_l) - w_z;
    if (a != a) return;
    if (a < -87.0f) return;  // w = 0: adds nothing
    const float w = det_expf(a) * kernel_weight * w_n;
    if (std::isinf(w) || std::isnan(w)) return;
    sum_color.x += color_p.x * w;
    sum_color.y += color_p.y * w;
    sum_color.z += color_p.z * w;
    sum_color.w += color_p.w * (w * w);
    sum_weight += w;
  }
};

static void subsampled(TapData& t, uint32_t iteration, int s) {
  if ((iteration & 1) == 0) {
    t.tap(-2 * s, 0, 1.0f);
    t.tap(2 * s, 0, 1.0f);
  } else {
    t.tap(0, -2 * s, 1.0f);
    t.tap(0, 2 * s, 1.0f);
  }
  t.tap(-1 * s, 1 * s, 1.0f);
  t.tap(1 * s, 1 * s, 1.0f);
  t.tap(-1 * s, -1 * s, 1.0f);
  t.tap(1 * s, -1 * s, 1.0f);
}
static void box(TapData& t, int r, int s) {
  for (int yy = -r; yy <= r; yy++)
    for (int xx = -r; xx <= r; xx++)
      if (xx != 0 || yy != 0) t.tap(xx * s, yy * s, 1.0f);
}
static void atrous(TapData& t, int s) {
  static const int order[24][2] = {{1, 0},  {0, 1},  {-1, 0},  {0, -1}, {2, 0},  {0, 2},  {-2, 0},  {0, -2}, {1, 1},  {-1, 1}, {-1, -1}, {1, -1},
                                   {1, 2},  {-1, 2}, {-1, -2}, {1, -2}, {2, 1},  {-2, 1}, {-2, -1}, {2, -1}, {2, 2},  {-2, 2}, {-2, -2}, {2, -2}};
  static const float weight[6] = {2.0f / 3.0f, 1.0f / 6.0f, 4.0f / 9.0f, 1.0f / 9.0f, 1.0f / 9.0f, 1.0f / 36.0f};
  for (int k = 0; k < 24; k++) t.tap(order[k][0] * s, order[k][1] * s, weight[k / 4]);
}

// atrous.hlsl:209-262
static void atrous_main(Problem& P, uint32_t iteration, int x, int y) {
  const int view = P.view_of(x, y);
  if (view == -1) return;
  const int step = 1 << iteration;
  const size_t i = P.at(x, y);
  TapData t;
  t.P = &P;
  t.input = &P.filter[iteration % 2];
  t.view_index = (uint32_t)view;
  t.ix = x;
  t.iy = y;
  t.step_size = step;
  t.center_normal = normal_of(P.visibility[i]);
  t.z_center = P.depth[i].z;
  t.dz_center[0] = P.depth[i].dz_dxy[0];
  t.dz_center[1] = P.depth[i].dz_dxy[1];
  t.sum_weight = 1;
  t.sum_color = (*t.input)[i];
  t.l_center = luminance(t.sum_color);
  t.compute_sigma_luminance();
  if (!std::isinf(t.z_center)) {
    switch (P.filter_type) {
      default:
      case 0: atrous(t, step); break;
      case 1: box(t, 1, step); break;
      case 2: box(t, 2, step); break;
      case 3: subsampled(t, iteration, step); break;
      case 4:
        if (step == 1)
          box(t, 1, step);
        else
          subsampled(t, iteration, step);
        break;
      case 5:
        if (step == 1)
          box(t, 2, step);
        else
          subsampled(t, iteration, step);
        break;
    }
  }
  const float inv_w = 1 / t.sum_weight;
  store(P.filter[(iteration + 1) % 2], i, Float4{t.sum_color.x * inv_w, t.sum_color.y * inv_w, t.sum_color.z * inv_w, t.sum_color.w * (inv_w * inv_w)});
}

template <typename T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
static bool write_image(FILE* f, const std::vector<Float4>& img) {
  if (!g_half) return fwrite(img.data(), sizeof(Float4), img.size(), f) == img.size();
  std::vector<uint16_t> h(4 * img.size());
  for (size_t i = 0; i < img.size(); i++) {
    h[4 * i + 0] = (uint16_t)det_f32tof16(img[i].x);
    h[4 * i + 1] = (uint16_t)det_f32tof16(img[i].y);
    h[4 * i + 2] = (uint16_t)det_f32tof16(img[i].z);
    h[4 * i + 3] = (uint16_t)det_f32tof16(img[i].w);
  }
  return fwrite(h.data(), 2, h.size(), f) == h.size();
}

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: denoise_ref <in> <out> [--half]\n");
    return 2;
  }
  g_half = argc > 3 && !strcmp(argv[3], "--half");
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  uint32_t h[12];
  if (fread(h, 4, 12, f) != 12 || memcmp(&h[0], "DNR1", 4) != 0) return 4;
  Problem P;
  P.width = h[1], P.height = h[2], P.view_count = h[3], P.instance_count = h[4], P.iterations = h[5], P.filter_type = h[6], P.history_tap = h[7];
  P.history_limit = det_u2f(h[8]), P.variance_boost_length = det_u2f(h[9]), P.sigma_luminance_boost = det_u2f(h[10]);
  const size_t n = (size_t)P.width * P.height;
  if (!read_n(f, P.views, P.view_count) || !read_n(f, P.visibility, n) || !read_n(f, P.depth, n) || !read_n(f, P.instance_index_map, P.instance_count) || !read_n(f, P.accum_color, n) ||
      !read_n(f, P.accum_moments, n) || !read_n(f, P.filter[0], n) || !read_n(f, P.filter[1], n))
    return 5;
  fclose(f);

  // Denoiser.cpp:215-265
  for (uint32_t y = 0; y < P.height; y++)
    for (uint32_t x = 0; x < P.width; x++) estimate_variance(P, (int)x, (int)y);
  for (uint32_t i = 0; i < P.iterations; i++) {
    for (uint32_t y = 0; y < P.height; y++)
      for (uint32_t x = 0; x < P.width; x++) atrous_main(P, i, (int)x, (int)y);
    if (i + 1 == P.history_tap)  // copy_rgb, atrous.hlsl:266-271
      for (size_t k = 0; k < n; k++) store(P.accum_color, k, Float4{P.filter[0][k].x, P.filter[0][k].y, P.filter[0][k].z, P.accum_color[k].w});
  }

  FILE* o = fopen(argv[2], "wb");
  if (!o) return 6;
  const bool ok = write_image(o, P.filter[0]) && write_image(o, P.filter[1]) && write_image(o, P.accum_color);
  return fclose(o) == 0 && ok ? 0 : 7;
}
