// top_level.h — sthip_scene_set_transforms (sthip.h): instance matrices as they lie in HBM, the derived inverse and motion
// matrices, the entry boxes of the top level with the host builder's arithmetic (bvh_build.cpp: rebuild_top_level), and a
// radix-tree top level over them, all on the device (top_level.hip). The functions below are the arithmetic contract; the
// kernels and the host path of the call (host builder with a derived array) both go through them.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/sthip.h"
#include "bvh.h"
#include "bvh_build.h"

namespace sthip {

// transform_inverse of the hosts (stratum_amd/scene.py, host/stratum_hip.hpp): adjugate over determinant in binary64 in this
// order, every quotient its own division, one rounding to binary32 at the store. false: the determinant is 0 or not finite.
STHIP_BVH_HD inline bool derive_inverse(const float* m /* 3x4 */, float* out /* 3x4 */) {
  const double a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[4], a11 = m[5], a12 = m[6], a20 = m[8], a21 = m[9], a22 = m[10];
  const double c00 = a11 * a22 - a12 * a21;
  const double c01 = a12 * a20 - a10 * a22;
  const double c02 = a10 * a21 - a11 * a20;
  const double det = a00 * c00 + a01 * c01 + a02 * c02;
  const double i[3][3] = {{c00 / det, (a02 * a21 - a01 * a22) / det, (a01 * a12 - a02 * a11) / det},
                          {c01 / det, (a00 * a22 - a02 * a20) / det, (a02 * a10 - a00 * a12) / det},
                          {c02 / det, (a01 * a20 - a00 * a21) / det, (a00 * a11 - a01 * a10) / det}};
  const double tx = m[3], ty = m[7], tz = m[11];
  for (int r = 0; r < 3; r++) {
    out[4 * r + 0] = (float)i[r][0];
    out[4 * r + 1] = (float)i[r][1];
    out[4 * r + 2] = (float)i[r][2];
    out[4 * r + 3] = (float)(0.0 - (i[r][0] * tx + i[r][1] * ty + i[r][2] * tz));
  }
  return det != 0.0 && det - det == 0.0;  // (finite and not zero)
}

// tmul of the hosts in binary32, rows dotted left to right: a * [b; 0 0 0 1]
STHIP_BVH_HD inline void derive_motion(const float* a, const float* b, float* out) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) {
      float s = a[4 * i + 0] * b[j] + a[4 * i + 1] * b[4 + j];
      s = s + a[4 * i + 2] * b[8 + j];
      if (j == 3) s = s + a[4 * i + 3];
      out[4 * i + j] = s;
    }
}

// is_identity of the builders: the twelve words compared as bits
STHIP_BVH_HD inline bool transform_is_identity(const float* m) {
  const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  for (int k = 0; k < 12; k++) {
    uint32_t x, y;
    memcpy(&x, &m[k], 4);
    memcpy(&y, &I[k], 4);
    if (x != y) return false;
  }
  return true;
}

STHIP_BVH_HD inline float tl_min(float a, float b) { return b < a ? b : a; }  // std::min / std::max of the host builder
STHIP_BVH_HD inline float tl_max(float a, float b) { return a < b ? b : a; }

// The world box of one entry, as rebuild_top_level computes it (bvh_build.cpp): `M` the instance's new transform, `obj_box`
// the entry's object-space bounds (transformed meshes), `vol` the entry's volume (volumes), `merged_box` the merged mesh's.
STHIP_BVH_HD inline void entry_world_box(const TlasEntry& e, const float* M, const float* obj_box, const DeviceVolume* vol, const float* merged_box, float lo[3], float hi[3]) {
  if (e.identity == TLAS_ENTRY_IDENTITY) {
    for (int a = 0; a < 3; a++) {
      lo[a] = merged_box[a];
      hi[a] = merged_box[3 + a];
    }
    return;
  }
  if (e.identity == TLAS_ENTRY_SPHERE) {
    const float r = fabsf(e.radius);
    for (int a = 0; a < 3; a++) {
      const float c = M[4 * a + 3];
      const float pad = 1e-3f * r + 1e-5f * fabsf(c);
      lo[a] = c - r - pad;
      hi[a] = c + r + pad;
    }
    return;
  }
  float corners[8][3];
  if (e.identity == TLAS_ENTRY_VOLUME) {
    const DeviceVolume& v = *vol;
    for (int c = 0; c < 8; c++) {
      const float ip[3] = {(float)((c & 1) ? v.bbox_max[0] + 1 : v.bbox_min[0]), (float)((c & 2) ? v.bbox_max[1] + 1 : v.bbox_min[1]), (float)((c & 4) ? v.bbox_max[2] + 1 : v.bbox_min[2])};
      for (int a = 0; a < 3; a++) corners[c][a] = ip[0] * v.matf[3 * a] + ip[1] * v.matf[3 * a + 1] + ip[2] * v.matf[3 * a + 2] + v.vecf[a];
    }
  } else {
    for (int c = 0; c < 8; c++)
      for (int a = 0; a < 3; a++) corners[c][a] = ((c >> a) & 1) ? obj_box[3 + a] : obj_box[a];
  }
  for (int a = 0; a < 3; a++) {
    lo[a] = INFINITY;
    hi[a] = -INFINITY;
  }
  for (int c = 0; c < 8; c++)
    for (int r = 0; r < 3; r++) {
      const float w = M[4 * r + 0] * corners[c][0] + M[4 * r + 1] * corners[c][1] + M[4 * r + 2] * corners[c][2] + M[4 * r + 3];
      lo[r] = tl_min(lo[r], w);
      hi[r] = tl_max(hi[r], w);
    }
  for (int a = 0; a < 3; a++) {
    const float m = tl_max(tl_max(fabsf(lo[a]), fabsf(hi[a])), hi[a] - lo[a]);
    const float pad = e.identity == TLAS_ENTRY_VOLUME ? 1e-3f * (hi[a] - lo[a]) + 1e-5f * tl_max(fabsf(lo[a]), fabsf(hi[a])) : 2e-5f * m;
    lo[a] -= pad;
    hi[a] += pad;
  }
}

// ---- the device side (top_level.hip) ----
#define TL_FLAG_MERGED_MOVED 1u  // an instance of the merged mesh whose new transform or inverse is not the identity
#define TL_FLAG_SINGULAR 2u      // a derived inverse whose determinant is 0 or not finite
#define TL_FLAG_BOX 4u           // an entry box that is not finite
struct TopLevelResult {          // the one read-back of a call
  uint32_t flags;
  uint32_t height;    // of the radix tree in inner nodes along the longest path (0: no tree)
  uint32_t box[6];    // the scene box: lo.xyz, hi.xyz as ordered integers (top_level_ord2f)
  uint32_t first_bad; // the lowest instance / entry index a flag was raised for (messages)
  uint32_t pad[3];
};
inline float top_level_ord2f(uint32_t u) {
  const uint32_t v = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
  float f;
  memcpy(&f, &v, 4);
  return f;
}

struct DeviceTopLevel;  // scratch and staging a context keeps between calls
DeviceTopLevel* device_top_level_create();
void device_top_level_destroy(DeviceTopLevel*);

struct TopLevelInputs {
  // the new matrices, device memory (the caller's arrays or the staging the host arrays went into); inv / motion may be NULL
  const sthip_TransformData *xf = nullptr, *inv = nullptr, *motion = nullptr;
  bool derive_motion = false;
  uint32_t instance_count = 0;
  // resident (all device): the transforms before the call, the entries, per-instance merged flags, object boxes, volumes
  const sthip_TransformData* resident_xf = nullptr;
  const TlasEntry* entries = nullptr;
  uint32_t entry_count = 0;
  const DeviceVolume* volumes = nullptr;
  uint32_t volume_count = 0;
  float merged_box[6] = {0, 0, 0, 0, 0, 0};
  uint32_t blas_nodes = 0;
  bool build_tree = true;  // false: boxes, entries and flags only (sthip_scene_read_top_level; a scene without a top level)
};
// the per-entry / per-instance tables the kernels read besides the resident arrays: uploaded when the resident tree changes
bool top_level_set_static(DeviceTopLevel*, const uint8_t* merged, uint32_t instance_count, const float* obj_box, uint32_t entry_count, void* stream, std::string& err);
// Enqueues everything on `stream` without a synchronisation in between, then copies the result record back and waits once.
// Nothing resident is written: the new matrices, entries and nodes lie in the staging of `tl` until top_level_install.
bool top_level_build(DeviceTopLevel* tl, const TopLevelInputs& in, void* stream, TopLevelResult& result, float& gpu_ms, std::string& err);
// device-to-device, in stream order: staging -> the resident arrays (any destination may be NULL: skipped)
bool top_level_install(DeviceTopLevel* tl, sthip_TransformData* xf, sthip_TransformData* inv, sthip_TransformData* motion, TlasEntry* entries, BvhNodeSlot* nodes /* + blas_nodes */, void* stream,
                       std::string& err);
// the staged results for the host: exact entry boxes (6 per entry), the unpacked nodes (entry_count - 1, or 1 for one entry)
bool top_level_read_boxes(DeviceTopLevel* tl, float* boxes, uint32_t entry_count, void* stream, std::string& err);
bool top_level_read_nodes(DeviceTopLevel* tl, BvhNode* nodes, uint32_t node_count, void* stream, std::string& err);

}  // namespace sthip
