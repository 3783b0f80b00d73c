// tri_test_parts_check.cpp — the two statements of the ray/triangle test in stratum_amd/csrc/tri_test.h against each other on
// the host: tri_edges(tri_shear(p0), tri_shear(p1), tri_shear(p2)) must return and write exactly what tri_whole(p0, p1, p2)
// does, bit for bit (a NaN equals any NaN; no accepted hit carries one), for random rays and triangles, triangles that share vertices, degenerate
// triangles, rays through vertices and along edges, huge, tiny, zero, infinite and NaN coordinates, and every axis
// permutation. Built with -ffp-contract=off, as the product is (tests/test_leaf_pairs.py).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../stratum_amd/csrc/tri_test.h"

static uint32_t state = 0x9E3779B9u;
static uint32_t next() {
  state ^= state << 13;
  state ^= state >> 17;
  state ^= state << 5;
  return state;
}
static float unit() { return (float)(next() >> 8) * (1.0f / 16777216.0f); }
static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
// Equal as bits — or both NaN: which NaN an operation on NaNs or inf * 0 gives (sign, payload) depends on the operand order the
// compiler picks for a commutative instruction, not on the statement; a test that returns true never wrote one (checked).
static bool same(float a, float b) { return bits(a) == bits(b) || (a != a && b != b); }
// a coordinate: mostly ordinary, sometimes one of the awkward values
static float coord() {
  static const float odd[] = {0.0f, -0.0f, 1.0f, -1.0f, 1e-38f, -1e-38f, 1e-45f, 3e38f, -3e38f, 1e19f, -1e19f, 1e-19f, std::numeric_limits<float>::infinity(),
                              -std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()};
  const uint32_t r = next() % 16u;
  if (r == 0) return odd[next() % (sizeof(odd) / sizeof(odd[0]))];
  if (r == 1) return (unit() * 2 - 1) * 1e6f;
  if (r == 2) return (unit() * 2 - 1) * 1e-6f;
  return unit() * 4 - 2;
}
// the shear constants of a direction, as traverse.h: setup_space makes them
static void shear_of(const float d[3], TriRay& s) {
  int kz = 0;
  float m = std::fabs(d[0]);
  if (std::fabs(d[1]) > m) kz = 1, m = std::fabs(d[1]);
  if (std::fabs(d[2]) > m) kz = 2;
  int kx = kz + 1 == 3 ? 0 : kz + 1, ky = kx + 1 == 3 ? 0 : kx + 1;
  if (d[kz] < 0.0f) {
    const int t = kx;
    kx = ky;
    ky = t;
  }
  s.k = kx | (ky << 2) | (kz << 4);
  s.Sx = d[kx] / d[kz];
  s.Sy = d[ky] / d[kz];
  s.Sz = 1.0f / d[kz];
}

int main() {
  size_t cases = 0, hits = 0;
  for (int n = 0; n < 400000; n++) {
    TriRay s;
    float d[3] = {coord(), coord(), coord()};
    s.ox = coord(), s.oy = coord(), s.oz = coord();
    shear_of(d, s);
    if (n % 7 == 0) {  // constants no direction gives: any permutation, any values
      s.k = (int)(next() % 3) | (int)(next() % 3) << 2 | (int)(next() % 3) << 4;
      s.Sx = coord(), s.Sy = coord(), s.Sz = coord();
    }
    TriV p[3];
    for (int k = 0; k < 3; k++) p[k] = TriV{coord(), coord(), coord()};
    switch (next() % 8u) {
      case 0: p[1] = p[0]; break;                                   // two equal vertices
      case 1: p[2] = p[1] = p[0]; break;                            // a point
      case 2: p[2] = TriV{2 * p[1].x - p[0].x, 2 * p[1].y - p[0].y, 2 * p[1].z - p[0].z}; break;  // collinear
      case 3: p[0] = TriV{s.ox + d[0], s.oy + d[1], s.oz + d[2]}; break;  // the ray goes through a vertex
      case 4: {                                                     // ... or along an edge's plane: a point of the edge on the ray
        const float w = unit();
        const TriV on = {s.ox + 2 * d[0], s.oy + 2 * d[1], s.oz + 2 * d[2]};
        p[1] = TriV{on.x + w * (on.x - p[0].x), on.y + w * (on.y - p[0].y), on.z + w * (on.z - p[0].z)};
        break;
      }
      case 5: {                                                     // the triangle moved so that the ray goes through its inside
        const float cx = (p[0].x + p[1].x + p[2].x) / 3, cy = (p[0].y + p[1].y + p[2].y) / 3, cz = (p[0].z + p[1].z + p[2].z) / 3;
        for (int k = 0; k < 3; k++) p[k] = TriV{p[k].x - cx + s.ox + 1.5f * d[0], p[k].y - cy + s.oy + 1.5f * d[1], p[k].z - cz + s.oz + 1.5f * d[2]};
        break;
      }
      default: break;
    }
    const float tmin = n % 5 == 0 ? coord() : 0.0f, tmax = n % 3 == 0 ? coord() : std::numeric_limits<float>::infinity();
    float t0 = 0, u0 = 0, v0 = 0, t1 = 0, u1 = 0, v1 = 0;
    const bool whole = tri_whole(s, p[0], p[1], p[2], tmin, tmax, t0, u0, v0);
    const bool parts = tri_edges(tri_shear(s, p[0]), tri_shear(s, p[1]), tri_shear(s, p[2]), tmin, tmax, t1, u1, v1);
    if (whole != parts || !same(t0, t1) || !same(u0, u1) || !same(v0, v1) || (whole && (t0 != t0 || u0 != u0 || v0 != v0))) {
      std::printf("FAIL: case %d: whole %d (%a %a %a), parts %d (%a %a %a)\n", n, (int)whole, t0, u0, v0, (int)parts, t1, u1, v1);
      return 1;
    }
    cases++;
    hits += whole;
  }
  if (hits < 1000) return std::printf("FAIL: only %zu of %zu cases hit: the inputs test nothing\n", hits, cases), 1;
  std::printf("TRI TEST PARTS OK %zu cases, %zu hits\n", cases, hits);
  return 0;
}
