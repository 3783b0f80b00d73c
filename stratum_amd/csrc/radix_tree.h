// radix_tree.h — Karras' radix tree over sorted 64-bit keys ("Maximizing Parallelism in the Construction of BVHs, Octrees, and
// k-d Trees", HPG 2012), shared by the triangle builder (lbvh.hip) and the top-level builder (top_level.hip). Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sthip {

// common-prefix length of the keys at sorted positions i and j; equal keys are told apart by position
__device__ __forceinline__ int radix_delta(const unsigned long long* keys, int n, int i, int j) {
  if (j < 0 || j >= n) return -1;
  const unsigned long long a = keys[i], b = keys[j];
  if (a == b) return 64 + __clz((uint32_t)i ^ (uint32_t)j);
  return __clzll(a ^ b);
}

// Karras 2012: internal node i (0 <= i < n - 1, one thread each) of the radix tree over n sorted keys; a child is an internal
// node index or 0x80000000 | sorted position of a leaf; node 0 is the root
__device__ __forceinline__ void radix_tree_node(const unsigned long long* keys, int n, int i, uint32_t* left, uint32_t* right, uint32_t* parent_of_internal, uint32_t* parent_of_leaf) {
  const int d = (radix_delta(keys, n, i, i + 1) - radix_delta(keys, n, i, i - 1)) >= 0 ? 1 : -1;
  const int dmin = radix_delta(keys, n, i, i - d);
  int lmax = 2;
  while (radix_delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
  int l = 0;
  for (int t = lmax / 2; t >= 1; t /= 2)
    if (radix_delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
  const int j = i + l * d;
  const int dnode = radix_delta(keys, n, i, j);
  int s = 0;
  int t = l;
  do {
    t = (t + 1) >> 1;
    if (radix_delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
  } while (t > 1);
  const int gamma = i + s * d + min(d, 0);
  const int lo = min(i, j), hi = max(i, j);
  const uint32_t L = (lo == gamma) ? (0x80000000u | (uint32_t)gamma) : (uint32_t)gamma;
  const uint32_t R = (hi == gamma + 1) ? (0x80000000u | (uint32_t)(gamma + 1)) : (uint32_t)(gamma + 1);
  left[i] = L;
  right[i] = R;
  if (L & 0x80000000u)
    parent_of_leaf[gamma] = (uint32_t)i;
  else
    parent_of_internal[gamma] = (uint32_t)i;
  if (R & 0x80000000u)
    parent_of_leaf[gamma + 1] = (uint32_t)i;
  else
    parent_of_internal[gamma + 1] = (uint32_t)i;
}

}  // namespace sthip
