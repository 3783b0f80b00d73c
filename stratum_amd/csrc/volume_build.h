// volume_build.h — a NanoVDB 32.3.3 float grid (FogVolume, background 0) from a dense box of binary32 values, built on the
// device (volume_build.hip): what the C ABI hands the build, and the layout both sides share. The contract is that of
// include/sthip.h (sthip_build_volume); its second statement is stratum_amd/nvdb.py.
#pragma once
#include <stdint.h>

#include <string>

namespace sthip {

// sizes of the published format (PNanoVDB.h, FLOAT row of the type constants; media.h reads by the same)
constexpr uint64_t NVDB_GRID_BYTES = 672, NVDB_TREE_BYTES = 64, NVDB_ROOT_BYTES = 64, NVDB_TILE_BYTES = 32, NVDB_UPPER_BYTES = 270400, NVDB_LOWER_BYTES = 33856, NVDB_LEAF_BYTES = 2144;
constexpr uint64_t NVDB_MAX_BYTES = 0xFFFFFFF0ull;  // DeviceVolume::bytes is 32 bits
constexpr uint32_t NVDB_MAX_TILES = 65536;          // the device reader walks the root's tile table linearly

struct VolumeBuildInput {
  const float* dense;  // device memory, dense[(x * ny + y) * nz + z]
  uint32_t dims[3];
  int32_t origin[3];
};

// the one read-back of a build: what decides every refusal, the allocation and the header
struct VolumeBuildCounts {
  uint32_t leaves, lowers, uppers, nonfinite;
  uint64_t active;
  int32_t bbox_min[3], bbox_max[3];
  float min, max;
};

struct VolumeLayout {  // byte offsets from the grid's first byte
  uint64_t root, upper, lower, leaf, total;
};
inline VolumeLayout volume_layout(const VolumeBuildCounts& c) {
  VolumeLayout l;
  l.root = NVDB_GRID_BYTES + NVDB_TREE_BYTES;
  l.upper = l.root + NVDB_ROOT_BYTES + NVDB_TILE_BYTES * c.uppers;
  l.lower = l.upper + NVDB_UPPER_BYTES * c.uppers;
  l.leaf = l.lower + NVDB_LOWER_BYTES * c.lowers;
  l.total = l.leaf + NVDB_LEAF_BYTES * c.leaves;
  return l;
}

// GridData, TreeData and the root's 64 bytes, made on the host from the read-back (the binary64 map and world box are
// host arithmetic: unfused products and sums)
struct VolumeHeader {
  uint32_t w[(NVDB_GRID_BYTES + NVDB_TREE_BYTES + NVDB_ROOT_BYTES) / 4];
};
void volume_header(const VolumeBuildCounts& c, double voxel_size, const double translation[3], const char* name, VolumeHeader& out, double world_bbox[6]);

// ---- layout order without a sort (device and host: tests/cpp/volume_slots_check.cpp checks it against a sort) ----
// Bricks are numbered by (upper cell, lower cell in it, brick in that), each x-major over the part of the cell the lattice
// covers. The lattice is a box, so the number is a closed form of the coordinate, and the children of a cell are consecutive.
#if defined(__HIPCC__)
#define STHIP_VB_HD __host__ __device__ __forceinline__
#else
#define STHIP_VB_HD inline
#endif

struct VbLattice {
  int32_t origin[3];
  uint32_t dims[3];
  int32_t b0[3];  // bricks: index >> 3
  uint32_t bn[3];
  int32_t m0[3];  // lower cells: index >> 7
  uint32_t mn[3];
  int32_t u0[3];  // upper cells: index >> 12
  uint32_t un[3];
  uint32_t bricks, lowers, uppers;
};

// false: more than VB_MAX_BRICKS bricks. The cap keeps the build's scratch (20 B per brick) at 336 MB and the one-workgroup
// prefix sum of volume_build.hip at 4 096 steps; a box of 2 048^3 voxels fits it exactly.
constexpr uint64_t VB_MAX_BRICKS = 1ull << 24;
inline bool vb_lattice(const VolumeBuildInput& in, VbLattice& L) {
  uint64_t cells[3] = {1, 1, 1};
  for (int a = 0; a < 3; a++) {
    L.origin[a] = in.origin[a];
    L.dims[a] = in.dims[a];
    const int64_t last = (int64_t)in.origin[a] + (int64_t)in.dims[a] - 1;
    L.b0[a] = in.origin[a] >> 3, L.bn[a] = (uint32_t)((last >> 3) - L.b0[a] + 1);
    L.m0[a] = in.origin[a] >> 7, L.mn[a] = (uint32_t)((last >> 7) - L.m0[a] + 1);
    L.u0[a] = in.origin[a] >> 12, L.un[a] = (uint32_t)((last >> 12) - L.u0[a] + 1);
    cells[0] *= L.bn[a], cells[1] *= L.mn[a], cells[2] *= L.un[a];
    if (cells[0] > VB_MAX_BRICKS) return false;
  }
  L.bricks = (uint32_t)cells[0], L.lowers = (uint32_t)cells[1], L.uppers = (uint32_t)cells[2];
  return true;
}

STHIP_VB_HD uint32_t vb_plain(const int32_t c[3], const int32_t lo[3], const uint32_t n[3]) {
  return ((uint32_t)(c[0] - lo[0]) * n[1] + (uint32_t)(c[1] - lo[1])) * n[2] + (uint32_t)(c[2] - lo[2]);
}
// The range [lo, lo + n) is cut down to the coarse cell (2^shift fine cells per axis) that holds c; returns how many fine
// cells of the range come before that part in the order (coarse cell x-major, then the cells inside it).
STHIP_VB_HD uint32_t vb_nest(const int32_t c[3], int shift, int32_t lo[3], uint32_t n[3]) {
  uint32_t before[3], cn[3];
  for (int a = 0; a < 3; a++) {
    const int32_t first = (c[a] >> shift) * (1 << shift), last = first + (1 << shift) - 1, end = lo[a] + (int32_t)n[a] - 1;
    const int32_t l = lo[a] > first ? lo[a] : first, h = end < last ? end : last;
    before[a] = (uint32_t)(l - lo[a]);
    cn[a] = (uint32_t)(h - l + 1);
    lo[a] = l;
  }
  const uint32_t r = before[0] * n[1] * n[2] + cn[0] * (before[1] * n[2] + cn[1] * before[2]);
  for (int a = 0; a < 3; a++) n[a] = cn[a];
  return r;
}
// slot of brick c in layout order; on return lo/n are the bricks of c's lower cell and `first` the slot of the first of them
STHIP_VB_HD uint32_t vb_brick_slot(const VbLattice& L, const int32_t c[3], int32_t lo[3], uint32_t n[3], uint32_t& first) {
  for (int a = 0; a < 3; a++) lo[a] = L.b0[a], n[a] = L.bn[a];
  first = vb_nest(c, 9, lo, n);
  first += vb_nest(c, 4, lo, n);
  return first + vb_plain(c, lo, n);
}
// slot of lower cell m; lo/n: the lower cells of m's upper cell, `first` the slot of the first of them
STHIP_VB_HD uint32_t vb_lower_slot(const VbLattice& L, const int32_t m[3], int32_t lo[3], uint32_t n[3], uint32_t& first) {
  for (int a = 0; a < 3; a++) lo[a] = L.m0[a], n[a] = L.mn[a];
  first = vb_nest(m, 5, lo, n);
  return first + vb_plain(m, lo, n);
}
STHIP_VB_HD void vb_unravel(uint32_t i, const int32_t lo[3], const uint32_t n[3], int32_t c[3]) {
  c[2] = lo[2] + (int32_t)(i % n[2]);
  i /= n[2];
  c[1] = lo[1] + (int32_t)(i % n[1]);
  c[0] = lo[0] + (int32_t)(i / n[1]);
}

struct DeviceVolumeBuild;
DeviceVolumeBuild* device_volume_build_create();
void device_volume_build_destroy(DeviceVolumeBuild* vb);

// The scan pass, the prefix sums and the node reductions, then the read-back (the stream is waited for). False with `err`
// on a HIP error or a lattice of more than VB_MAX_BRICKS bricks.
bool volume_build_scan(DeviceVolumeBuild* vb, const VolumeBuildInput& in, void* stream, VolumeBuildCounts& counts, float& gpu_ms, std::string& err);
// The emit passes of the grid the last scan described, into `out` (device memory, 32-byte aligned, volume_layout().total
// bytes): every byte of the grid is written. The stream is waited for.
bool volume_build_emit(DeviceVolumeBuild* vb, const VolumeBuildInput& in, const VolumeBuildCounts& counts, const VolumeHeader& header, void* out, void* stream, float& gpu_ms, std::string& err);
// a staging area of the build's own for a grid that goes to host memory (grows, keeps its capacity)
void* volume_build_staging(DeviceVolumeBuild* vb, uint64_t bytes, std::string& err);

}  // namespace sthip
