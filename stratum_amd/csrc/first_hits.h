// first_hits.h — what the first bounce of a view pass depends on (host only, no HIP: tests/cpp/first_hit_key_check.cpp
// compiles it alone).
//
// k_generate shoots the primary ray of a path slot through the centre of its pixel: no jitter, no random number. The closest
// hit is a function of the ray and the triangles alone (the hit contract), so p.hit / p.hit_leaf after k_trace_primary are
// the same bytes for every seed of a call and for every call, as long as nothing below changes. sthip_render keeps them in
// two buffers of the context ("reuse_first_hits", api.hip: run_batches) and launches the packet kernel only when the key of
// the call differs from the key the kept hits were traced for.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/sthip_wire.h"

namespace sthip {

// Calls with more views than this keep nothing (the key is a plain struct of fixed size)
constexpr uint32_t FIRST_HITS_MAX_VIEWS = 8;

// Everything the ray / meta outputs of k_generate and the hits of k_trace_primary read, by reader:
//   slot_to_pixel      paths_per_seed, tile_w, tile_h, shard_count, shard_rank, gOutputExtent (and tiles_x / tiles_y, which
//                      follow from the extent and the tile size)
//   get_view_index     gViewCount, image_min / image_max of every view
//   k_generate         gMaxPathVertices < 2 (no ray, the slot is dead); the view's transform (the origin is its translation)
//   primary_dir        the view's projection, image_min / image_max, the view's transform
//   k_trace_primary    ray_o / ray_d / meta (the above), the tree, its triangles, the instances' entries, and under
//                      alpha_test the alpha masks, the triangles' uvs and flip_uvs: the resident scene, which only the
//                      entry points that bump the context's serial number change (sthip_scene_upload and the rebuilds it
//                      serves, sthip_scene_update_transforms, sthip_scene_update_vertices / sthip_scene_animate,
//                      sthip_scene_set_rigs); hit_leaf is an index into the resident leaf-triangle array, so a rebuild
//                      of the same triangles counts too
// The views and their transforms are compared as bytes (the whole records: fields no kernel above reads only cost a trace
// that was not needed). The seed, the sampling flags other than the two named, the outputs and the path budget beyond
// "at least 2 vertices" are not in it: the first bounce does not read them.
struct FirstHitKey {
  uint64_t scene_serial;
  uint32_t extent[2];   // gOutputExtent
  uint32_t view_count;  // gViewCount
  uint32_t traced;      // gMaxPathVertices >= 2
  uint32_t shard_rank, shard_count, tile_w, tile_h;
  uint32_t paths_per_seed;
  uint32_t alpha_test, flip_uvs;  // DeviceBvh::alpha_test / flip_uvs of the call
  sthip_ViewData views[FIRST_HITS_MAX_VIEWS];          // [0, view_count); the rest is zero
  sthip_TransformData view_xf[FIRST_HITS_MAX_VIEWS];   // likewise
};

// Fills `k`; reads exactly view_count records of each array. False (and a key that equals nothing, itself included) when the
// call cannot be described: no views, more than FIRST_HITS_MAX_VIEWS, a missing array.
inline bool first_hit_key_make(FirstHitKey& k, uint64_t scene_serial, const uint32_t extent[2], uint32_t view_count, uint32_t max_path_vertices, uint32_t shard_rank, uint32_t shard_count, uint32_t tile_w,
                               uint32_t tile_h, uint32_t paths_per_seed, bool alpha_test, bool flip_uvs, const sthip_ViewData* views, const sthip_TransformData* view_xf) {
  memset(&k, 0, sizeof(k));
  if (view_count == 0 || view_count > FIRST_HITS_MAX_VIEWS || !views || !view_xf) return false;
  k.scene_serial = scene_serial;
  k.extent[0] = extent[0];
  k.extent[1] = extent[1];
  k.view_count = view_count;
  k.traced = max_path_vertices >= 2 ? 1u : 0u;
  k.shard_rank = shard_rank;
  k.shard_count = shard_count;
  k.tile_w = tile_w;
  k.tile_h = tile_h;
  k.paths_per_seed = paths_per_seed;
  k.alpha_test = alpha_test ? 1u : 0u;
  k.flip_uvs = flip_uvs ? 1u : 0u;
  memcpy(k.views, views, (size_t)view_count * sizeof(sthip_ViewData));
  memcpy(k.view_xf, view_xf, (size_t)view_count * sizeof(sthip_TransformData));
  return true;
}

inline bool first_hit_key_equal(const FirstHitKey& a, const FirstHitKey& b) {
  if (a.view_count == 0 || a.view_count > FIRST_HITS_MAX_VIEWS || a.view_count != b.view_count) return false;  // (a key that was never made describes no call)
  return a.scene_serial == b.scene_serial && a.extent[0] == b.extent[0] && a.extent[1] == b.extent[1] && a.traced == b.traced && a.shard_rank == b.shard_rank && a.shard_count == b.shard_count &&
         a.tile_w == b.tile_w && a.tile_h == b.tile_h && a.paths_per_seed == b.paths_per_seed && a.alpha_test == b.alpha_test && a.flip_uvs == b.flip_uvs &&
         !memcmp(a.views, b.views, (size_t)a.view_count * sizeof(sthip_ViewData)) && !memcmp(a.view_xf, b.view_xf, (size_t)a.view_count * sizeof(sthip_TransformData));
}

}  // namespace sthip
