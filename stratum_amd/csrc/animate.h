// animate.h — rigs posed on the device (animate.hip): what api.hip hands the one kernel that writes gVertices.
#pragma once

#include <stdint.h>

#include <string>

#include "../../include/sthip.h"

namespace sthip {

constexpr uint32_t ANIMATE_MAX_TARGETS = 4;    // anim.hlsl:12-15: four blend target bindings
constexpr uint32_t ANIMATE_MAX_BONES = 1024;   // 1024 x 48 B = 48 KB of LDS per block

// One rig as it is resident: all pointers are device pointers; `vertices`, `rest`, `targets[k]` and `weights` point at the
// rig's first record and hold vertex_count records each. `bones` holds bone_count matrices.
struct AnimateRig {
  sthip_PackedVertexData* vertices = nullptr;  // gVertices + first_vertex: written
  const sthip_PackedVertexData* rest = nullptr;
  const sthip_PackedVertexData* targets[ANIMATE_MAX_TARGETS] = {nullptr, nullptr, nullptr, nullptr};
  const sthip_VertexWeight* weights = nullptr;
  const sthip_TransformData* bones = nullptr;
  uint32_t vertex_count = 0, target_count = 0, bone_count = 0;
  float factors[ANIMATE_MAX_TARGETS] = {0, 0, 0, 0};  // (of absent targets: 0)
};

// Enqueues k_animate for one rig (nothing for an empty one).
bool animate_launch(const AnimateRig& rig, int cu_count, void* stream, std::string& err);

}  // namespace sthip
