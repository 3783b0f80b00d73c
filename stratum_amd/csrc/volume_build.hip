// volume_build.hip — a NanoVDB 32.3.3 float grid from a dense box of binary32 values, on the device. The contract is that of
// include/sthip.h (sthip_build_volume): a voxel is active iff its value != 0; a node exists iff it has an active voxel; root
// tiles ascend by signed tile coordinate, the nodes of a level follow their parents and then the child index; min, max and the
// index boxes are exact at every level; nothing is pruned. stratum_amd/nvdb.py states the same in numpy and is equalled byte
// for byte.
//
// The build is level-synchronous: kernel boundaries are the only ordering, no fence, flag or spin inside a launch.
//   k_vb_scan        one wave64 per 8^3 brick of the leaf lattice the box touches; a lane owns one (x, y) row of 8 z-contiguous
//                    values (two 16-byte loads where the row lies inside the box and is 16-byte aligned, else per element).
//                    Writes per brick its active count, min, max and active box; reductions stay within the wave.
//   k_vb_rank        exclusive prefix sum of "has an active voxel" in layout order: every node's index in its level.
//   k_vb_reduce      one wave per lower cell over its bricks, then one wave per upper cell over its lower cells.
//   k_vb_root        one wave: ranks of the upper nodes (the root tiles), the root's box, min and max, the counts read back.
//   (the read-back; the host decides every refusal, the size and the header)
//   k_vb_emit_leaves one wave per brick again: the values go straight from the dense array into the leaf as 16-byte groups.
//   k_vb_emit_nodes  one workgroup per lower cell, then per upper cell: masks, child offsets, box, min/max.
//   k_vb_emit_root   the tile table; GridData, TreeData and the root's 64 bytes from the host's header.
// Layout order without a sort: bricks are numbered by (upper cell, lower cell in it, brick in that), each x-major over the
// part of the cell the lattice covers; the lattice is a box, so the number is a closed form of the coordinate (vb_brick_slot),
// and the children of a cell are consecutive slots.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "volume_build.h"

namespace sthip {
namespace {

#define VB_DEV __device__ __forceinline__

struct VbBrick {
  uint32_t count;       // active voxels
  uint32_t kmin, kmax;  // ordered keys of min and max (vb_key)
  uint32_t box;         // local active box: min x, y, z then max x, y, z, 3 bits each
};
struct VbNode {
  uint32_t count;  // children with an active voxel
  uint32_t kmin, kmax;
  int32_t lo[3], hi[3];
  uint64_t active;
};
struct VbHead {
  VolumeBuildCounts res;
};

// binary32 bits -> an unsigned key with the order of the values (no arithmetic on the values: subnormals stay what they are)
VB_DEV uint32_t vb_key(uint32_t bits) { return bits ^ ((uint32_t)((int32_t)bits >> 31) | 0x80000000u); }
VB_DEV uint32_t vb_unkey(uint32_t k) { return k ^ ((k & 0x80000000u) ? 0x80000000u : 0xFFFFFFFFu); }

// The row of 8 values lane `lane` owns in brick c: x = lane >> 3, y = lane & 7, z = 0..7. Outside the box: 0.
VB_DEV void vb_load_row(const float* __restrict__ dense, const VbLattice& L, const int32_t c[3], uint32_t lane, uint32_t v[8]) {
  for (int k = 0; k < 8; k++) v[k] = 0u;
  const int64_t x = (int64_t)c[0] * 8 + (int64_t)(lane >> 3) - L.origin[0], y = (int64_t)c[1] * 8 + (int64_t)(lane & 7u) - L.origin[1], z0 = (int64_t)c[2] * 8 - L.origin[2];
  if (x < 0 || x >= (int64_t)L.dims[0] || y < 0 || y >= (int64_t)L.dims[1]) return;
  const uint64_t row = ((uint64_t)x * L.dims[1] + (uint64_t)y) * L.dims[2];
  if (z0 >= 0 && z0 + 8 <= (int64_t)L.dims[2] && (((uintptr_t)(dense + row + (uint64_t)z0)) & 15u) == 0) {
    const uint4* p = reinterpret_cast<const uint4*>(dense + row + (uint64_t)z0);
    const uint4 a = p[0], b = p[1];
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
    return;
  }
  const uint32_t* p = reinterpret_cast<const uint32_t*>(dense) + row;
  for (int k = 0; k < 8; k++) {
    const int64_t z = z0 + k;
    if (z >= 0 && z < (int64_t)L.dims[2]) v[k] = p[z];
  }
}

VB_DEV uint32_t vb_wave_min(uint32_t v) {
  for (int s = 32; s > 0; s >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, s, 64));
  return v;
}
VB_DEV uint32_t vb_wave_max(uint32_t v) {
  for (int s = 32; s > 0; s >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, s, 64));
  return v;
}
VB_DEV uint32_t vb_wave_sum(uint32_t v) {
  for (int s = 32; s > 0; s >>= 1) v += (uint32_t)__shfl_xor((int)v, s, 64);
  return v;
}
VB_DEV int32_t vb_wave_imin(int32_t v) {
  for (int s = 32; s > 0; s >>= 1) v = min(v, __shfl_xor(v, s, 64));
  return v;
}
VB_DEV int32_t vb_wave_imax(int32_t v) {
  for (int s = 32; s > 0; s >>= 1) v = max(v, __shfl_xor(v, s, 64));
  return v;
}

constexpr uint32_t VB_BLOCK = 256, VB_WAVES = VB_BLOCK / 64;

// ---- the scan pass ----
__global__ __launch_bounds__(VB_BLOCK) void k_vb_scan(const float* __restrict__ dense, VbLattice L, VbBrick* __restrict__ bricks, VbHead* head) {
  const uint32_t b = blockIdx.x * VB_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (b >= L.bricks) return;  // (wave-uniform)
  int32_t c[3], lo[3];
  uint32_t n[3], first;
  vb_unravel(b, L.b0, L.bn, c);
  uint32_t v[8];
  vb_load_row(dense, L, c, lane, v);
  uint32_t byte = 0, kmin = 0xFFFFFFFFu, kmax = 0u, bad = 0u;
  for (int k = 0; k < 8; k++) {
    bad |= (v[k] & 0x7F800000u) == 0x7F800000u ? 1u : 0u;
    if (v[k] & 0x7FFFFFFFu) {
      byte |= 1u << k;
      const uint32_t key = vb_key(v[k]);
      kmin = min(kmin, key);
      kmax = max(kmax, key);
    }
  }
  const unsigned long long rows = __ballot(byte != 0);  // bit x * 8 + y
  const unsigned long long any_bad = __ballot(bad != 0);
  const uint32_t count = vb_wave_sum(__popc(byte));
  kmin = vb_wave_min(kmin);
  kmax = vb_wave_max(kmax);
  uint32_t zbits = 0;
  for (int k = 0; k < 8; k++) zbits |= __ballot((byte >> k) & 1u) ? 1u << k : 0u;
  if (lane != 0) return;
  if (any_bad) atomicOr(&head->res.nonfinite, 1u);
  VbBrick r;
  r.count = count, r.kmin = kmin, r.kmax = kmax, r.box = 0;
  if (count) {
    uint32_t ybits = 0;
    for (int x = 0; x < 8; x++) ybits |= (uint32_t)(rows >> (8 * x)) & 0xFFu;
    const uint32_t x0 = (uint32_t)__builtin_ctzll(rows) >> 3, x1 = (63u - (uint32_t)__builtin_clzll(rows)) >> 3;
    const uint32_t y0 = (uint32_t)__builtin_ctz(ybits), y1 = 31u - (uint32_t)__builtin_clz(ybits);
    const uint32_t z0 = (uint32_t)__builtin_ctz(zbits), z1 = 31u - (uint32_t)__builtin_clz(zbits);
    r.box = x0 | (y0 << 3) | (z0 << 6) | (x1 << 9) | (y1 << 12) | (z1 << 15);
  }
  bricks[vb_brick_slot(L, c, lo, n, first)] = r;
}

// ---- prefix sums: one workgroup walks the level, 4 records per thread and step ----
constexpr uint32_t VB_RANK_BLOCK = 1024, VB_RANK_ITEMS = 4;
template <typename Rec>
__global__ __launch_bounds__(VB_RANK_BLOCK) void k_vb_rank(const Rec* __restrict__ recs, uint32_t n, uint32_t* __restrict__ rank, uint32_t* total) {
  __shared__ uint32_t wave_sum[VB_RANK_BLOCK / 64];
  __shared__ uint32_t carry;
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  if (t == 0) carry = 0;
  __syncthreads();
  for (uint32_t base = 0; base < n; base += VB_RANK_BLOCK * VB_RANK_ITEMS) {
    const uint32_t i0 = base + t * VB_RANK_ITEMS;
    uint32_t f[VB_RANK_ITEMS], mine = 0;
    for (uint32_t k = 0; k < VB_RANK_ITEMS; k++) {
      f[k] = (i0 + k < n && recs[i0 + k].count) ? 1u : 0u;
      mine += f[k];
    }
    uint32_t incl = mine;  // inclusive sum over the wave
    for (int s = 1; s < 64; s <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, s, 64);
      if ((int)lane >= s) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t before = carry;
    for (uint32_t w = 0; w < wave; w++) before += wave_sum[w];
    uint32_t r = before + incl - mine;
    for (uint32_t k = 0; k < VB_RANK_ITEMS; k++) {
      if (i0 + k < n) rank[i0 + k] = r;
      r += f[k];
    }
    __syncthreads();
    if (t == VB_RANK_BLOCK - 1) carry = before + incl;
    __syncthreads();
  }
  if (t == 0) *total = carry;
}

// ---- a cell's record from its children (LEVEL 0: a lower cell over its bricks; 1: an upper cell over its lower cells) ----
template <int LEVEL>
__global__ __launch_bounds__(VB_BLOCK) void k_vb_reduce(VbLattice L, const VbBrick* __restrict__ bricks, const VbNode* __restrict__ lowers, VbNode* __restrict__ out) {
  const uint32_t cell = blockIdx.x * VB_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (cell >= (LEVEL == 0 ? L.lowers : L.uppers)) return;  // (wave-uniform)
  int32_t c[3], lo[3], cc[3];
  uint32_t n[3], first, slot;
  if (LEVEL == 0) {
    vb_unravel(cell, L.m0, L.mn, c);
    int32_t plo[3];
    uint32_t pn[3], pfirst;
    slot = vb_lower_slot(L, c, plo, pn, pfirst);
    for (int a = 0; a < 3; a++) cc[a] = max(L.b0[a], c[a] * 16);  // the first brick of the cell that the lattice covers
    vb_brick_slot(L, cc, lo, n, first);
  } else {
    vb_unravel(cell, L.u0, L.un, c);
    slot = cell;  // (upper cells are x-major already: the order of the root tiles)
    for (int a = 0; a < 3; a++) cc[a] = max(L.m0[a], c[a] * 32);
    vb_lower_slot(L, cc, lo, n, first);
  }
  const uint32_t children = n[0] * n[1] * n[2];
  uint32_t count = 0, kmin = 0xFFFFFFFFu, kmax = 0u;
  int32_t blo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, bhi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  uint64_t active = 0;
  for (uint32_t i = lane; i < children; i += 64) {
    if (LEVEL == 0) {
      const VbBrick r = bricks[first + i];
      if (!r.count) continue;
      int32_t bc[3];
      vb_unravel(i, lo, n, bc);
      count++, active += r.count, kmin = min(kmin, r.kmin), kmax = max(kmax, r.kmax);
      for (int a = 0; a < 3; a++) {
        blo[a] = min(blo[a], bc[a] * 8 + (int32_t)((r.box >> (3 * a)) & 7u));
        bhi[a] = max(bhi[a], bc[a] * 8 + (int32_t)((r.box >> (9 + 3 * a)) & 7u));
      }
    } else {
      const VbNode r = lowers[first + i];
      if (!r.count) continue;
      count++, active += r.active, kmin = min(kmin, r.kmin), kmax = max(kmax, r.kmax);
      for (int a = 0; a < 3; a++) blo[a] = min(blo[a], r.lo[a]), bhi[a] = max(bhi[a], r.hi[a]);
    }
  }
  VbNode r;
  r.count = vb_wave_sum(count);
  r.kmin = vb_wave_min(kmin), r.kmax = vb_wave_max(kmax);
  for (int a = 0; a < 3; a++) r.lo[a] = vb_wave_imin(blo[a]), r.hi[a] = vb_wave_imax(bhi[a]);
  const uint32_t alo = vb_wave_sum((uint32_t)(active & 0xFFFFu)), amid = vb_wave_sum((uint32_t)((active >> 16) & 0xFFFFu)), ahi = vb_wave_sum((uint32_t)(active >> 32));
  r.active = (uint64_t)alo + ((uint64_t)amid << 16) + ((uint64_t)ahi << 32);  // (64 addends of 16 bits each: no carry is lost)
  if (lane == 0) out[slot] = r;
}

// ---- the root: ranks of the upper nodes in tile order, the grid's box, min, max and counts ----
__global__ __launch_bounds__(64) void k_vb_root(VbLattice L, const VbNode* __restrict__ uppers, uint32_t* __restrict__ upper_rank, const uint32_t* leaf_total, const uint32_t* lower_total, VbHead* head) {
  const uint32_t lane = threadIdx.x;
  uint32_t ranked = 0, kmin = 0xFFFFFFFFu, kmax = 0u;
  int32_t blo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, bhi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  uint64_t active = 0;
  for (uint32_t base = 0; base < L.uppers; base += 64) {
    const uint32_t u = base + lane;
    bool has = false;
    if (u < L.uppers) {
      const VbNode r = uppers[u];
      has = r.count != 0;
      if (has) {
        active += r.active, kmin = min(kmin, r.kmin), kmax = max(kmax, r.kmax);
        for (int a = 0; a < 3; a++) blo[a] = min(blo[a], r.lo[a]), bhi[a] = max(bhi[a], r.hi[a]);
      }
    }
    const unsigned long long m = __ballot(has);
    if (u < L.uppers) upper_rank[u] = ranked + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    ranked += (uint32_t)__popcll(m);
  }
  kmin = vb_wave_min(kmin), kmax = vb_wave_max(kmax);
  for (int a = 0; a < 3; a++) blo[a] = vb_wave_imin(blo[a]), bhi[a] = vb_wave_imax(bhi[a]);
  uint64_t total = 0;  // (a sum of 64-bit counts: one lane walks the 64 partial sums)
  for (int l = 0; l < 64; l++) total += ((uint64_t)(uint32_t)__shfl((int)(active >> 32), l, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)active, l, 64);
  if (lane != 0) return;
  VolumeBuildCounts& r = head->res;
  r.leaves = *leaf_total, r.lowers = *lower_total, r.uppers = ranked;
  r.active = total;
  for (int a = 0; a < 3; a++) r.bbox_min[a] = blo[a], r.bbox_max[a] = bhi[a];
  r.min = __uint_as_float(vb_unkey(kmin)), r.max = __uint_as_float(vb_unkey(kmax));
}

// ---- emit: leaves ----
__global__ __launch_bounds__(VB_BLOCK) void k_vb_emit_leaves(const float* __restrict__ dense, VbLattice L, const VbBrick* __restrict__ bricks, const uint32_t* __restrict__ leaf_rank, uint8_t* __restrict__ out,
                                                           uint64_t leaf_off) {
  const uint32_t b = blockIdx.x * VB_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (b >= L.bricks) return;
  int32_t c[3], lo[3];
  uint32_t n[3], first;
  vb_unravel(b, L.b0, L.bn, c);
  const uint32_t slot = vb_brick_slot(L, c, lo, n, first);
  const VbBrick r = bricks[slot];
  if (!r.count) return;  // (wave-uniform)
  uint32_t v[8];
  vb_load_row(dense, L, c, lane, v);
  uint32_t byte = 0;
  for (int k = 0; k < 8; k++) {
    if (v[k] & 0x7FFFFFFFu)
      byte |= 1u << k;
    else
      v[k] = 0u;  // (-0.0f is inactive and reads back as +0)
  }
  uint32_t* leaf = reinterpret_cast<uint32_t*>(out + leaf_off + NVDB_LEAF_BYTES * (uint64_t)leaf_rank[slot]);
  // the 96 bytes ahead of the values, one word per lane: bbox_min, bbox_dif | flags, the 512-bit mask, min, max, average, deviation
  uint32_t mask_word = 0;
  for (int k = 0; k < 4; k++) mask_word |= (uint32_t)__shfl((int)byte, (int)((4u * (lane - 4u) + k) & 63u), 64) << (8 * k);
  uint32_t word = 0;
  if (lane < 3)
    word = (uint32_t)((lane == 0 ? c[0] : lane == 1 ? c[1] : c[2]) * 8 + (int32_t)((r.box >> (3 * lane)) & 7u));
  else if (lane == 3)
    word = (((r.box >> 9) & 7u) - (r.box & 7u)) | ((((r.box >> 12) & 7u) - ((r.box >> 3) & 7u)) << 8) | ((((r.box >> 15) & 7u) - ((r.box >> 6) & 7u)) << 16) | (2u << 24);
  else if (lane < 20)
    word = mask_word;
  else if (lane == 20)
    word = vb_unkey(r.kmin);
  else if (lane == 21)
    word = vb_unkey(r.kmax);
  if (lane < 24) leaf[lane] = word;
  uint4* values = reinterpret_cast<uint4*>(leaf + 24 + 8 * lane);
  values[0] = make_uint4(v[0], v[1], v[2], v[3]);
  values[1] = make_uint4(v[4], v[5], v[6], v[7]);
}

// ---- emit: lower (LEVEL 0) and upper (LEVEL 1) nodes, one workgroup per cell ----
template <int LEVEL>
__global__ __launch_bounds__(VB_BLOCK) void k_vb_emit_nodes(VbLattice L, const VbBrick* __restrict__ bricks, const VbNode* __restrict__ lowers, const VbNode* __restrict__ uppers, const uint32_t* __restrict__ child_rank,
                                                          const uint32_t* __restrict__ self_rank, uint8_t* __restrict__ out, uint64_t self_off, uint64_t child_off) {
  constexpr uint32_t LOG2 = LEVEL == 0 ? 4 : 5, TABLE = 1u << (3 * LOG2), MASK_WORDS = TABLE / 32;
  constexpr uint64_t SELF_BYTES = LEVEL == 0 ? NVDB_LOWER_BYTES : NVDB_UPPER_BYTES, CHILD_BYTES = LEVEL == 0 ? NVDB_LEAF_BYTES : NVDB_LOWER_BYTES;
  const uint32_t cell = blockIdx.x, t = threadIdx.x;
  int32_t c[3], lo[3], cc[3];
  uint32_t n[3], first, slot;
  if (LEVEL == 0) {
    vb_unravel(cell, L.m0, L.mn, c);
    int32_t plo[3];
    uint32_t pn[3], pfirst;
    slot = vb_lower_slot(L, c, plo, pn, pfirst);
    for (int a = 0; a < 3; a++) cc[a] = max(L.b0[a], c[a] * 16);
    vb_brick_slot(L, cc, lo, n, first);
  } else {
    vb_unravel(cell, L.u0, L.un, c);
    slot = cell;
    for (int a = 0; a < 3; a++) cc[a] = max(L.m0[a], c[a] * 32);
    vb_lower_slot(L, cc, lo, n, first);
  }
  const VbNode self = LEVEL == 0 ? lowers[slot] : uppers[slot];
  if (!self.count) return;  // (uniform over the workgroup)
  const uint64_t self_byte = self_off + SELF_BYTES * (uint64_t)self_rank[slot];
  uint32_t* node = reinterpret_cast<uint32_t*>(out + self_byte);
  // bbox (6 words), flags (2), value mask: all zero, there are no active tiles; child mask: below
  for (uint32_t w = t; w < 8 + MASK_WORDS; w += VB_BLOCK)
    node[w] = w == 0 ? (uint32_t)self.lo[0] : w == 1 ? (uint32_t)self.lo[1] : w == 2 ? (uint32_t)self.lo[2] : w == 3 ? (uint32_t)self.hi[0] : w == 4 ? (uint32_t)self.hi[1] : w == 5 ? (uint32_t)self.hi[2] : w == 6 ? 2u : 0u;
  // min, max, average, deviation and 16 bytes of padding behind the masks
  uint32_t* stats = node + 8 + 2 * MASK_WORDS;
  if (t < 8) stats[t] = t == 0 ? vb_unkey(self.kmin) : t == 1 ? vb_unkey(self.kmax) : 0u;
  unsigned long long* child_mask = reinterpret_cast<unsigned long long*>(node + 8 + MASK_WORDS);
  long long* table = reinterpret_cast<long long*>(stats + 8);
  for (uint32_t e = t; e < TABLE; e += VB_BLOCK) {  // (TABLE is a multiple of the workgroup: whole waves to the end)
    int32_t k[3] = {c[0] * (1 << LOG2) + (int32_t)(e >> (2 * LOG2)), c[1] * (1 << LOG2) + (int32_t)((e >> LOG2) & ((1u << LOG2) - 1u)), c[2] * (1 << LOG2) + (int32_t)(e & ((1u << LOG2) - 1u))};
    long long entry = 0;
    bool inside = true;
    for (int a = 0; a < 3; a++) inside = inside && k[a] >= lo[a] && k[a] < lo[a] + (int32_t)n[a];
    if (inside) {
      const uint32_t child = first + vb_plain(k, lo, n);
      const bool has = LEVEL == 0 ? bricks[child].count != 0 : lowers[child].count != 0;
      if (has) entry = (long long)(child_off + CHILD_BYTES * (uint64_t)child_rank[child]) - (long long)self_byte;  // relative to the node itself
    }
    table[e] = entry;  // (a tile's value: 0)
    const unsigned long long m = __ballot(entry != 0);
    if ((t & 63u) == 0) child_mask[e >> 6] = m;
  }
}

// ---- emit: the root's tiles, and the header the host made ----
__global__ __launch_bounds__(VB_BLOCK) void k_vb_emit_root(VbLattice L, const VbNode* __restrict__ uppers, const uint32_t* __restrict__ upper_rank, VolumeHeader header, uint8_t* __restrict__ out, uint64_t root_off,
                                                         uint64_t upper_off) {
  const uint32_t i = blockIdx.x * VB_BLOCK + threadIdx.x;
  if (i < sizeof(VolumeHeader) / 4) reinterpret_cast<uint32_t*>(out)[i] = header.w[i];
  if (i >= L.uppers || !uppers[i].count) return;
  int32_t c[3];
  vb_unravel(i, L.u0, L.un, c);
  const uint32_t rank = upper_rank[i];
  const unsigned long long key = (unsigned long long)((uint32_t)c[2] & 0xFFFFFu) | ((unsigned long long)((uint32_t)c[1] & 0xFFFFFu) << 21) | ((unsigned long long)((uint32_t)c[0] & 0xFFFFFu) << 42);
  unsigned long long* tile = reinterpret_cast<unsigned long long*>(out + root_off + NVDB_ROOT_BYTES + NVDB_TILE_BYTES * (uint64_t)rank);
  tile[0] = key;
  tile[1] = upper_off + NVDB_UPPER_BYTES * (uint64_t)rank - root_off;  // relative to the root
  tile[2] = 0;  // state (a child: unused), value 0
  tile[3] = 0;
}

// a device array that grows and keeps its capacity between calls (new memory is poisoned under STHIP_POISON_ALLOC, as every
// buffer of the context is)
template <typename T>
struct VbBuf {
  T* p = nullptr;
  size_t n = 0;
  hipError_t ensure(size_t count) {
    if (count <= n && p) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    if (count == 0) return hipSuccess;
    hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
    if (e == hipSuccess) n = count;
    static const int poison = [] {
      const char* v = getenv("STHIP_POISON_ALLOC");
      return v && *v ? (int)(strtoul(v, nullptr, 0) & 0xFFu) : -1;
    }();
    if (e == hipSuccess && poison >= 0) e = hipMemset(p, poison, count * sizeof(T));
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
};

}  // namespace

struct DeviceVolumeBuild {
  VbBuf<VbHead> head;
  VbBuf<uint32_t> totals;  // leaves, lower nodes
  VbBuf<VbBrick> bricks;
  VbBuf<VbNode> lowers, uppers;
  VbBuf<uint32_t> leaf_rank, lower_rank, upper_rank;
  VbBuf<uint8_t> staging;
  hipEvent_t ev[2] = {nullptr, nullptr};
  VbLattice lattice;  // of the last scan
  bool scanned = false;
};

DeviceVolumeBuild* device_volume_build_create() { return new DeviceVolumeBuild(); }
void device_volume_build_destroy(DeviceVolumeBuild* vb) {
  if (!vb) return;
  vb->head.release();
  vb->totals.release();
  vb->bricks.release();
  vb->lowers.release();
  vb->uppers.release();
  vb->leaf_rank.release();
  vb->lower_rank.release();
  vb->upper_rank.release();
  vb->staging.release();
  for (int k = 0; k < 2; k++)
    if (vb->ev[k]) (void)hipEventDestroy(vb->ev[k]);
  delete vb;
}

#define VB_TRY(expr)                                                              \
  do {                                                                            \
    const hipError_t e_ = (expr);                                                 \
    if (e_ != hipSuccess) {                                                       \
      err = std::string("volume build: ") + hipGetErrorString(e_) + " (" #expr ")"; \
      return false;                                                               \
    }                                                                             \
  } while (0)

static inline uint32_t vb_grid(uint32_t n, uint32_t per_block) { return std::max(1u, (n + per_block - 1) / per_block); }

bool volume_build_scan(DeviceVolumeBuild* vb, const VolumeBuildInput& in, void* stream_, VolumeBuildCounts& counts, float& gpu_ms, std::string& err) {
  hipStream_t stream = (hipStream_t)stream_;
  gpu_ms = 0;
  vb->scanned = false;
  VbLattice& L = vb->lattice;
  if (!vb_lattice(in, L)) {
    err = "volume build: the box touches more than 2^24 bricks of 8^3 voxels";
    return false;
  }
  // ---- reserve ----
  VB_TRY(vb->head.ensure(1));
  VB_TRY(vb->totals.ensure(2));
  VB_TRY(vb->bricks.ensure(L.bricks));
  VB_TRY(vb->leaf_rank.ensure(L.bricks));
  VB_TRY(vb->lowers.ensure(L.lowers));
  VB_TRY(vb->lower_rank.ensure(L.lowers));
  VB_TRY(vb->uppers.ensure(L.uppers));
  VB_TRY(vb->upper_rank.ensure(L.uppers));
  for (int k = 0; k < 2; k++)
    if (!vb->ev[k]) VB_TRY(hipEventCreate(&vb->ev[k]));
  // ---- enqueue ----
  VB_TRY(hipEventRecord(vb->ev[0], stream));
  VB_TRY(hipMemsetAsync(vb->head.p, 0, sizeof(VbHead), stream));
  hipLaunchKernelGGL(k_vb_scan, dim3(vb_grid(L.bricks, VB_WAVES)), dim3(VB_BLOCK), 0, stream, in.dense, L, vb->bricks.p, vb->head.p);
  hipLaunchKernelGGL(k_vb_rank<VbBrick>, dim3(1), dim3(VB_RANK_BLOCK), 0, stream, vb->bricks.p, L.bricks, vb->leaf_rank.p, vb->totals.p);
  hipLaunchKernelGGL(k_vb_reduce<0>, dim3(vb_grid(L.lowers, VB_WAVES)), dim3(VB_BLOCK), 0, stream, L, vb->bricks.p, (const VbNode*)nullptr, vb->lowers.p);
  hipLaunchKernelGGL(k_vb_rank<VbNode>, dim3(1), dim3(VB_RANK_BLOCK), 0, stream, vb->lowers.p, L.lowers, vb->lower_rank.p, vb->totals.p + 1);
  hipLaunchKernelGGL(k_vb_reduce<1>, dim3(vb_grid(L.uppers, VB_WAVES)), dim3(VB_BLOCK), 0, stream, L, vb->bricks.p, vb->lowers.p, vb->uppers.p);
  hipLaunchKernelGGL(k_vb_root, dim3(1), dim3(64), 0, stream, L, vb->uppers.p, vb->upper_rank.p, vb->totals.p, vb->totals.p + 1, vb->head.p);
  VB_TRY(hipGetLastError());
  VB_TRY(hipEventRecord(vb->ev[1], stream));
  // ---- the one read-back ----
  VB_TRY(hipMemcpyAsync(&counts, &vb->head.p->res, sizeof(VolumeBuildCounts), hipMemcpyDeviceToHost, stream));
  VB_TRY(hipStreamSynchronize(stream));
  (void)hipEventElapsedTime(&gpu_ms, vb->ev[0], vb->ev[1]);
  vb->scanned = true;
  return true;
}

bool volume_build_emit(DeviceVolumeBuild* vb, const VolumeBuildInput& in, const VolumeBuildCounts& counts, const VolumeHeader& header, void* out_, void* stream_, float& gpu_ms, std::string& err) {
  hipStream_t stream = (hipStream_t)stream_;
  gpu_ms = 0;
  if (!vb->scanned) {
    err = "volume build: no scan to emit from";
    return false;
  }
  const VbLattice& L = vb->lattice;
  const VolumeLayout lay = volume_layout(counts);
  uint8_t* out = (uint8_t*)out_;
  VB_TRY(hipEventRecord(vb->ev[0], stream));
  hipLaunchKernelGGL(k_vb_emit_leaves, dim3(vb_grid(L.bricks, VB_WAVES)), dim3(VB_BLOCK), 0, stream, in.dense, L, vb->bricks.p, vb->leaf_rank.p, out, lay.leaf);
  hipLaunchKernelGGL(k_vb_emit_nodes<0>, dim3(L.lowers), dim3(VB_BLOCK), 0, stream, L, vb->bricks.p, vb->lowers.p, vb->uppers.p, vb->leaf_rank.p, vb->lower_rank.p, out, lay.lower, lay.leaf);
  hipLaunchKernelGGL(k_vb_emit_nodes<1>, dim3(L.uppers), dim3(VB_BLOCK), 0, stream, L, vb->bricks.p, vb->lowers.p, vb->uppers.p, vb->lower_rank.p, vb->upper_rank.p, out, lay.upper, lay.lower);
  hipLaunchKernelGGL(k_vb_emit_root, dim3(vb_grid(std::max<uint32_t>(L.uppers, sizeof(VolumeHeader) / 4), VB_BLOCK)), dim3(VB_BLOCK), 0, stream, L, vb->uppers.p, vb->upper_rank.p, header, out, lay.root, lay.upper);
  VB_TRY(hipGetLastError());
  VB_TRY(hipEventRecord(vb->ev[1], stream));
  VB_TRY(hipStreamSynchronize(stream));
  (void)hipEventElapsedTime(&gpu_ms, vb->ev[0], vb->ev[1]);
  return true;
}

void* volume_build_staging(DeviceVolumeBuild* vb, uint64_t bytes, std::string& err) {
  const hipError_t e = vb->staging.ensure((size_t)bytes);
  if (e != hipSuccess) {
    err = std::string("volume build: ") + hipGetErrorString(e) + " (staging)";
    return nullptr;
  }
  return vb->staging.p;
}

void volume_header(const VolumeBuildCounts& c, double voxel_size, const double translation[3], const char* name, VolumeHeader& out, double world_bbox[6]) {
  uint8_t* b = (uint8_t*)out.w;
  memset(b, 0, sizeof(out));
  auto put = [&](size_t off, const void* v, size_t n) { memcpy(b + off, v, n); };
  auto put32 = [&](size_t off, uint32_t v) { put(off, &v, 4); };
  auto put64 = [&](size_t off, uint64_t v) { put(off, &v, 8); };
  auto putf = [&](size_t off, float v) { put(off, &v, 4); };
  auto putd = [&](size_t off, double v) { put(off, &v, 8); };
  const VolumeLayout lay = volume_layout(c);
  // GridData (PNanoVDB.h:761-777)
  put64(0, 0x304244566f6e614eull);   // magic
  put64(8, 0xFFFFFFFFFFFFFFFFull);   // checksum: none
  put32(16, 0x04000c03u);            // 32.3.3
  put32(20, 0x26u);                  // bounding boxes, min/max, breadth first
  put32(24, 0), put32(28, 1);        // grid 0 of 1
  put64(32, lay.total);
  if (name) put(40, name, std::min<size_t>(strlen(name), 255));
  const double inv = 1.0 / voxel_size;
  const size_t map = 296;  // (PNanoVDB.h:702-711)
  for (int k = 0; k < 3; k++) {
    putf(map + 4 * (4 * k), (float)voxel_size);
    putf(map + 36 + 4 * (4 * k), (float)inv);
    putf(map + 72 + 4 * k, (float)translation[k]);
    putd(map + 88 + 8 * (4 * k), voxel_size);
    putd(map + 160 + 8 * (4 * k), inv);
    putd(map + 232 + 8 * k, translation[k]);
    world_bbox[k] = (double)c.bbox_min[k] * voxel_size + translation[k];
    world_bbox[3 + k] = ((double)c.bbox_max[k] + 1.0) * voxel_size + translation[k];
    putd(608 + 8 * k, voxel_size);
  }
  putf(map + 84, 1.0f), putd(map + 256, 1.0);  // tapers
  for (int k = 0; k < 6; k++) putd(560 + 8 * k, world_bbox[k]);
  put32(632, 2), put32(636, 1);  // FogVolume, float; no blind data
  // TreeData (PNanoVDB.h:904-916): offsets from the tree, node counts, no tiles, the active voxels
  const size_t tree = NVDB_GRID_BYTES;
  put64(tree + 0, lay.leaf - tree), put64(tree + 8, lay.lower - tree), put64(tree + 16, lay.upper - tree), put64(tree + 24, lay.root - tree);
  put32(tree + 32, c.leaves), put32(tree + 36, c.lowers), put32(tree + 40, c.uppers);
  put64(tree + 56, c.active);
  // the root (PNanoVDB.h:964-968): box, table size, background 0, min, max, average 0, deviation 0
  const size_t root = (size_t)lay.root;
  for (int k = 0; k < 3; k++) put32(root + 4 * k, (uint32_t)c.bbox_min[k]), put32(root + 12 + 4 * k, (uint32_t)c.bbox_max[k]);
  put32(root + 24, c.uppers);
  putf(root + 32, c.min), putf(root + 36, c.max);
}

}  // namespace sthip
