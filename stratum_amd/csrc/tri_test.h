// tri_test.h — the watertight ray/triangle test (Woop, Benthin, Wald 2013), arithmetic exactly as the hit contract states
// (include/sthip.h): edge functions are products rounded separately (no fma) so that a shared edge evaluates
// antisymmetrically. Plain C++ on floats, so that the device (traverse.h: TRI_FN = __device__ __forceinline__) and a host
// check (tests/cpp/tri_test_parts_check.cpp) compile the same text. Two statements of one test:
//   tri_whole    three vertices at once — what every kernel that reads BvhTri runs;
//   tri_shear + tri_edges   the per-vertex part (the vertex relative to the origin, sheared: Ax, Ay and the scaled Az) and the
//                per-triangle part on three sheared vertices — a leaf whose triangles share vertices shears each vertex once
//                (Traversal::pair_step). Same operations on the same operands as tri_whole, so the same bits: the host check
//                compares the two over random and degenerate inputs.
#pragma once
#include <math.h>

#ifndef TRI_FN
#define TRI_FN static inline
#endif

struct TriRay {  // the ray's part: origin in the triangles' space, shear constants, axis permutation kx | ky << 2 | kz << 4
  float ox, oy, oz;
  float Sx, Sy, Sz;
  int k;
};
struct TriV {
  float x, y, z;
};
TRI_FN float tri_comp(TriV v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : v.z); }

TRI_FN bool tri_whole(const TriRay& s, TriV p0, TriV p1, TriV p2, float tmin, float tmax, float& t, float& b1, float& b2) {
  const TriV A = {p0.x - s.ox, p0.y - s.oy, p0.z - s.oz}, B = {p1.x - s.ox, p1.y - s.oy, p1.z - s.oz}, C = {p2.x - s.ox, p2.y - s.oy, p2.z - s.oz};
  const int kx = s.k & 3, ky = (s.k >> 2) & 3, kz = s.k >> 4;
  const float Akz = tri_comp(A, kz), Bkz = tri_comp(B, kz), Ckz = tri_comp(C, kz);
  const float Ax = fmaf(-s.Sx, Akz, tri_comp(A, kx)), Ay = fmaf(-s.Sy, Akz, tri_comp(A, ky));
  const float Bx = fmaf(-s.Sx, Bkz, tri_comp(B, kx)), By = fmaf(-s.Sy, Bkz, tri_comp(B, ky));
  const float Cx = fmaf(-s.Sx, Ckz, tri_comp(C, kx)), Cy = fmaf(-s.Sy, Ckz, tri_comp(C, ky));
  const float U = Cx * By - Cy * Bx;
  const float V = Ax * Cy - Ay * Cx;
  const float W = Bx * Ay - By * Ax;
  // No early exits: in a wave every lane waits for the slowest one anyway, and each `return` would cost an exec-mask
  // region (the tests are the same, in the same arithmetic; a zero determinant makes rcp infinite and tt fail its range
  // test, or NaN, which fails it too — det != 0 is tested all the same).
  const bool edges_disagree = ((U < 0.0f) | (V < 0.0f) | (W < 0.0f)) & ((U > 0.0f) | (V > 0.0f) | (W > 0.0f));
  const float det = U + V + W;
  const float Az = s.Sz * Akz, Bz = s.Sz * Bkz, Cz = s.Sz * Ckz;
  const float T = fmaf(W, Cz, fmaf(V, Bz, U * Az));
  const float rcp = 1.0f / det;
  const float tt = T * rcp;
  t = tt;
  b1 = V * rcp;
  b2 = W * rcp;
  return !edges_disagree & (det != 0.0f) & (tt > tmin) & (tt < tmax);
}

TRI_FN TriV tri_shear(const TriRay& s, TriV p) {
  const TriV A = {p.x - s.ox, p.y - s.oy, p.z - s.oz};
  const int kx = s.k & 3, ky = (s.k >> 2) & 3, kz = s.k >> 4;
  const float Akz = tri_comp(A, kz);
  const TriV r = {fmaf(-s.Sx, Akz, tri_comp(A, kx)), fmaf(-s.Sy, Akz, tri_comp(A, ky)), s.Sz * Akz};
  return r;
}
TRI_FN bool tri_edges(TriV a, TriV b, TriV c, float tmin, float tmax, float& t, float& b1, float& b2) {
  const float U = c.x * b.y - c.y * b.x;
  const float V = a.x * c.y - a.y * c.x;
  const float W = b.x * a.y - b.y * a.x;
  const bool edges_disagree = ((U < 0.0f) | (V < 0.0f) | (W < 0.0f)) & ((U > 0.0f) | (V > 0.0f) | (W > 0.0f));
  const float det = U + V + W;
  const float T = fmaf(W, c.z, fmaf(V, b.z, U * a.z));
  const float rcp = 1.0f / det;
  const float tt = T * rcp;
  t = tt;
  b1 = V * rcp;
  b2 = W * rcp;
  return !edges_disagree & (det != 0.0f) & (tt > tmin) & (tt < tmax);
}
