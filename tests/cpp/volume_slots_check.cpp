// volume_slots_check.cpp — the layout order of the device volume build (stratum_amd/csrc/volume_build.h: vb_brick_slot,
// vb_lower_slot) against a sort: for a list of boxes, every brick's slot is its rank under the key (index >> 12, index >> 7,
// index >> 3) per axis, x first; every lower cell's slot likewise; and the children of a cell are the consecutive slots the
// emit kernels take them for. Host only.
//   volume_slots_check      prints "ok <boxes>" and returns 0, or says what differs
#include <algorithm>
#include <array>
#include <cstdio>
#include <vector>

#include "../../stratum_amd/csrc/volume_build.h"

using namespace sthip;

static int check(const int32_t origin[3], const uint32_t dims[3]) {
  VolumeBuildInput in{};
  for (int a = 0; a < 3; a++) in.origin[a] = origin[a], in.dims[a] = dims[a];
  VbLattice L;
  if (!vb_lattice(in, L)) return std::printf("lattice refused\n"), 1;
  // bricks
  std::vector<std::array<int32_t, 9>> keys;
  std::vector<std::array<int32_t, 3>> coords;
  for (uint32_t b = 0; b < L.bricks; b++) {
    int32_t c[3];
    vb_unravel(b, L.b0, L.bn, c);
    coords.push_back({c[0], c[1], c[2]});
    keys.push_back({c[0] >> 9, c[1] >> 9, c[2] >> 9, c[0] >> 4, c[1] >> 4, c[2] >> 4, c[0], c[1], c[2]});
  }
  std::vector<uint32_t> order(L.bricks);
  for (uint32_t b = 0; b < L.bricks; b++) order[b] = b;
  std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return keys[x] < keys[y]; });
  for (uint32_t rank = 0; rank < L.bricks; rank++) {
    const auto& c = coords[order[rank]];
    int32_t lo[3];
    uint32_t n[3], first;
    const uint32_t slot = vb_brick_slot(L, c.data(), lo, n, first);
    if (slot != rank) return std::printf("brick (%d %d %d): slot %u, rank %u\n", c[0], c[1], c[2], slot, rank), 1;
    // the cell's range: every brick of it lies in [first, first + n), in x-major order
    if (slot != first + vb_plain(c.data(), lo, n) || first + n[0] * n[1] * n[2] > L.bricks) return std::printf("brick (%d %d %d): range\n", c[0], c[1], c[2]), 1;
    for (int a = 0; a < 3; a++)
      if ((lo[a] >> 4) != (c[a] >> 4) || ((lo[a] + (int32_t)n[a] - 1) >> 4) != (c[a] >> 4)) return std::printf("brick (%d %d %d): the range leaves the lower cell\n", c[0], c[1], c[2]), 1;
    int32_t cc[3] = {std::max(L.b0[0], (c[0] >> 4) * 16), std::max(L.b0[1], (c[1] >> 4) * 16), std::max(L.b0[2], (c[2] >> 4) * 16)};
    int32_t lo2[3];
    uint32_t n2[3], first2;
    if (vb_brick_slot(L, cc, lo2, n2, first2) != first || first2 != first) return std::printf("brick (%d %d %d): first of the cell\n", c[0], c[1], c[2]), 1;
  }
  // lower cells
  std::vector<std::array<int32_t, 6>> mkeys;
  std::vector<std::array<int32_t, 3>> mcoords;
  for (uint32_t m = 0; m < L.lowers; m++) {
    int32_t c[3];
    vb_unravel(m, L.m0, L.mn, c);
    mcoords.push_back({c[0], c[1], c[2]});
    mkeys.push_back({c[0] >> 5, c[1] >> 5, c[2] >> 5, c[0], c[1], c[2]});
  }
  std::vector<uint32_t> morder(L.lowers);
  for (uint32_t m = 0; m < L.lowers; m++) morder[m] = m;
  std::sort(morder.begin(), morder.end(), [&](uint32_t x, uint32_t y) { return mkeys[x] < mkeys[y]; });
  for (uint32_t rank = 0; rank < L.lowers; rank++) {
    const auto& c = mcoords[morder[rank]];
    int32_t lo[3];
    uint32_t n[3], first;
    const uint32_t slot = vb_lower_slot(L, c.data(), lo, n, first);
    if (slot != rank || slot != first + vb_plain(c.data(), lo, n) || first + n[0] * n[1] * n[2] > L.lowers) return std::printf("lower cell (%d %d %d): slot %u, rank %u\n", c[0], c[1], c[2], slot, rank), 1;
  }
  return 0;
}

int main() {
  const struct {
    int32_t o[3];
    uint32_t d[3];
  } boxes[] = {
      {{0, 0, 0}, {1, 1, 1}},          {{-5, 3, 4090}, {13, 9, 21}},      {{0, 0, 0}, {8, 8, 300}},        {{0, 0, 0}, {24, 24, 24}},       {{-12, -14, -11}, {28, 28, 28}},
      {{-130, 120, 4000}, {270, 20, 200}}, {{4090, -4100, -3}, {10, 10, 140}}, {{-2147483647 - 1, 2147483000, 0}, {40, 600, 3}}, {{100, 100, 100}, {300, 150, 140}}, {{-4097, -129, -9}, {4200, 140, 20}},
  };
  int n = 0;
  for (const auto& b : boxes) {
    if (check(b.o, b.d)) return std::printf("box %d\n", n), 1;
    n++;
  }
  std::printf("ok %d\n", n);
  return 0;
}
