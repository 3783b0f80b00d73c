// texel_decode_ref.cpp — a scalar restatement of the texel decode, written from the contract in include/sthip.h
// (sthip_texel_format) and from nothing else: no file of csrc/ is included, only det_powf of include/sthip_detmath.h.
// Build: g++ -std=c++17 -O2 -ffp-contract=off texel_decode_ref.cpp
//   texel_decode_ref decode IN OUT   IN: uint32 format, width, height, then the image's bytes. OUT: width * height * 4 floats.
//   texel_decode_ref srgb IN OUT     IN: binary32 values c. OUT: the sRGB curve of each (what the numpy statement cannot state
//                                    itself: det_powf).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/sthip_detmath.h"

static float srgb(float c) { return c <= 0.04045f ? c / 12.92f : det_powf((c + 0.055f) / 1.055f, 2.4f); }

// the colour block at p[0 .. 8), texel t; `bc1`: the endpoints decide between the four- and the three-colour rule
static void colour_block(const uint8_t* p, unsigned t, bool bc1, float rgb[3]) {
  const unsigned c[2] = {(unsigned)p[0] | (unsigned)p[1] << 8, (unsigned)p[2] | (unsigned)p[3] << 8};
  const uint32_t bits = (uint32_t)p[4] | (uint32_t)p[5] << 8 | (uint32_t)p[6] << 16 | (uint32_t)p[7] << 24;
  const unsigned index = (bits >> (2 * t)) & 3;
  const bool four = !bc1 || c[0] > c[1];
  for (int k = 0; k < 3; k++) {
    const unsigned e0 = k == 0 ? c[0] >> 11 : k == 1 ? (c[0] >> 5) & 63 : c[0] & 31;
    const unsigned e1 = k == 0 ? c[1] >> 11 : k == 1 ? (c[1] >> 5) & 63 : c[1] & 31;
    const bool green = k == 1;
    float v;
    if (index == 0)
      v = (float)e0 / (green ? 63.0f : 31.0f);
    else if (index == 1)
      v = (float)e1 / (green ? 63.0f : 31.0f);
    else if (four)
      v = index == 2 ? (float)(2 * e0 + e1) / (green ? 189.0f : 93.0f) : (float)(e0 + 2 * e1) / (green ? 189.0f : 93.0f);
    else
      v = index == 2 ? (float)(e0 + e1) / (green ? 126.0f : 62.0f) : 0.0f;
    rgb[k] = v;
  }
}

// the RGTC block at p[0 .. 8), texel t
static float rgtc_block(const uint8_t* p, unsigned t) {
  const unsigned r0 = p[0], r1 = p[1];
  uint64_t bits = 0;
  for (int k = 0; k < 6; k++) bits |= (uint64_t)p[2 + k] << (8 * k);
  const unsigned i = (unsigned)(bits >> (3 * t)) & 7;
  if (i == 0) return (float)r0 / 255.0f;
  if (i == 1) return (float)r1 / 255.0f;
  if (r0 > r1) return (float)((8 - i) * r0 + (i - 1) * r1) / 1785.0f;
  if (i <= 5) return (float)((6 - i) * r0 + (i - 1) * r1) / 1275.0f;
  return i == 6 ? 0.0f : 1.0f;
}

static bool decode(unsigned f, unsigned w, unsigned h, const std::vector<uint8_t>& image, std::vector<float>& out) {
  if (f == 0) f = 31;
  if (f == 1) f = 19;
  if (f < 16 || f >= 40) return false;
  out.assign((size_t)w * h * 4, 0.0f);
  for (unsigned y = 0; y < h; y++)
    for (unsigned x = 0; x < w; x++) {
      float v[4] = {0.0f, 0.0f, 0.0f, 1.0f};
      bool curve = false;
      if (f < 32) {
        const unsigned cls = (f - 16) / 4, n = (f - 16) % 4 + 1;
        const size_t texel = (size_t)y * w + x;
        for (unsigned k = 0; k < n; k++) {
          if (cls <= 1) {
            v[k] = (float)image.at(texel * n + k) / 255.0f;
          } else if (cls == 2) {
            const unsigned lo = image.at((texel * n + k) * 2), hi = image.at((texel * n + k) * 2 + 1);
            v[k] = (float)(lo | hi << 8) / 65535.0f;
          } else {
            (void)image.at((texel * n + k) * 4 + 3);
            memcpy(&v[k], &image[(texel * n + k) * 4], 4);
          }
        }
        curve = cls == 1;
      } else {
        const unsigned size = (f == 32 || f == 37 || f == 35) ? 8 : 16;
        const size_t at = ((size_t)(y / 4) * ((w + 3) / 4) + x / 4) * size;
        (void)image.at(at + size - 1);
        const uint8_t* p = &image[at];
        const unsigned t = 4 * (y % 4) + x % 4;
        if (f == 32 || f == 37) {
          colour_block(p, t, true, v);
        } else if (f == 33 || f == 38) {
          colour_block(p + 8, t, false, v);
          v[3] = (float)((p[t / 2] >> (4 * (t % 2))) & 15) / 15.0f;
        } else if (f == 34 || f == 39) {
          colour_block(p + 8, t, false, v);
          v[3] = rgtc_block(p, t);
        } else if (f == 35) {
          v[0] = rgtc_block(p, t);
        } else {
          v[0] = rgtc_block(p, t);
          v[1] = rgtc_block(p + 8, t);
        }
        curve = f >= 37;
      }
      if (curve) {  // colour channels only; an absent channel is not a colour that was stored, but its 0 maps to 0 either way
        for (int k = 0; k < 3; k++) v[k] = srgb(v[k]);
      }
      memcpy(&out[((size_t)y * w + x) * 4], v, 16);
    }
  return true;
}

static bool read_file(const char* path, std::vector<uint8_t>& bytes) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  bytes.resize(n > 0 ? (size_t)n : 0);
  const bool ok = bytes.empty() || fread(bytes.data(), 1, bytes.size(), f) == bytes.size();
  fclose(f);
  return ok;
}

static bool write_file(const char* path, const std::vector<float>& v) {
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  const bool ok = v.empty() || fwrite(v.data(), 4, v.size(), f) == v.size();
  return fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
  if (argc != 4 || (strcmp(argv[1], "decode") && strcmp(argv[1], "srgb"))) {
    fprintf(stderr, "usage: texel_decode_ref decode|srgb IN OUT\n");
    return 2;
  }
  std::vector<uint8_t> in;
  if (!read_file(argv[2], in)) return 1;
  std::vector<float> out;
  if (!strcmp(argv[1], "srgb")) {
    out.resize(in.size() / 4);
    if (!out.empty()) memcpy(out.data(), in.data(), out.size() * 4);
    for (float& c : out) c = srgb(c);
  } else {
    if (in.size() < 12) return 1;
    uint32_t head[3];
    memcpy(head, in.data(), 12);
    if (!head[1] || !head[2] || (uint64_t)head[1] * head[2] > (1u << 24)) return 1;
    const std::vector<uint8_t> image(in.begin() + 12, in.end());
    if (!decode(head[0], head[1], head[2], image, out)) return 1;
  }
  return write_file(argv[3], out) ? 0 : 1;
}
