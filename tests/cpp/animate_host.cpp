// animate_host.cpp — a rig is posed between two frames of the C++ host (stratum_amd/host/stratum_hip.hpp): every mesh gets
// a rig through MeshPrimitive::set_rig before the first frame (one blend target, two bones) and a pose through set_pose
// after it; the scene is marked dirty, Scene::update repacks, and BDPT::update must find that only poses changed and pose
// the meshes on the device (sthip_scene_animate) instead of uploading: last_update_was_vertices_only().
//   animate_host <scene.bin> <out.bin> <seeds>          (GPU) writes the SECOND frame: RGBA32F radiance, prev-uv, ray counts
//   animate_host --host-pose <scene.bin> <vertices.bin> (no GPU) packs the posed scene with Scene::set_pose_on_device(false)
//                                                       and writes its vertex records: the host's fallback arithmetic
// The rig depends on a record's own contents only, in binary32 operations a numpy host reproduces exactly: the target is
// y += 0.04 * (x * z) with the rest pose's normals; bone 0 is the identity, bone 1 scales by 0.875 and translates by
// (0.0625, 0, 0.03125); every vertex has weights (0.75, 0.25, 0, 0) on bones (0, 1, 1, 0); the pose's factor is 0.5.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <unordered_set>

#include "../../stratum_amd/host/stratum_hip.hpp"
#include "scene_reader.hpp"

using namespace stm;

template <typename F>
static uint32_t for_each_mesh(Node& scene_node, F&& f) {  // every mesh once (instances may share one), through the primitive that carries it
  std::unordered_set<const Mesh*> done;
  uint32_t count = 0;
  scene_node.root().for_each_descendant<MeshPrimitive>([&](const component_ptr<MeshPrimitive>& prim) {
    if (!prim->mMesh || !done.insert(prim->mMesh.get()).second) return;
    f(*prim);
    count++;
  });
  return count;
}

static void set_rig(MeshPrimitive& prim) {
  Mesh::BlendTarget t;
  t.positions = prim.mMesh->positions;
  t.normals = prim.mMesh->normals;
  t.normals.resize(t.positions.size(), float3{});
  for (float3& q : t.positions) {
    const float xz = q.x * q.z;
    const float d = 0.04f * xz;
    q.y = q.y + d;
  }
  sthip_VertexWeight w{};
  w.weights[0] = 0.75f, w.weights[1] = 0.25f;
  w.indices[0] = 0, w.indices[1] = 1, w.indices[2] = 1, w.indices[3] = 0;
  prim.set_rig({t}, std::vector<sthip_VertexWeight>(t.positions.size(), w), 2);
}

static void set_pose(MeshPrimitive& prim) {
  std::vector<TransformData> bones(2, TransformData{});
  bones[0].m[0][0] = bones[0].m[1][1] = bones[0].m[2][2] = 1.0f;
  bones[1].m[0][0] = bones[1].m[1][1] = bones[1].m[2][2] = 0.875f;
  bones[1].m[0][3] = 0.0625f, bones[1].m[2][3] = 0.03125f;
  prim.set_pose({0.5f, 0.0f, 0.0f, 0.0f}, bones);
}

int main(int argc, char** argv) {
  const bool host_pose = argc >= 2 && !std::strcmp(argv[1], "--host-pose");
  if (argc < 4) {
    std::fprintf(stderr, "usage: animate_host scene.bin out.bin seeds | animate_host --host-pose scene.bin vertices.bin\n");
    return 2;
  }
  try {
    Reader r(argv[host_pose ? 2 : 1]);
    NodeGraph graph;
    Node& root = graph.emplace("Instance");
    auto app = root.make_child("Application").make_component<Application>();
    LoadedScene L = load_scene(r, app.node());
    auto scene = L.scene;
    CommandBuffer cb;
    if (host_pose) {
      for_each_mesh(*L.scene_node, [](MeshPrimitive& prim) { set_rig(prim), set_pose(prim); });
      scene->set_pose_on_device(false);
      scene->update(cb, 0.0f);
      if (!scene->data()->mRigs.empty()) return std::printf("a scene posed on the host carries no rigs\n"), 1;
      const auto& v = scene->data()->mVertices;
      std::ofstream out(argv[3], std::ios::binary);
      out.write((const char*)v.data(), v.size() * sizeof(v[0]));
      std::printf("HOST POSED vertices=%zu\n", v.size());
      return 0;
    }
    const ViewData view = L.view;
    const TransformData view_xf = L.view_xf;
    const uint32_t W = L.W, H = L.H;
    const uint32_t seeds = (uint32_t)std::atoi(argv[3]);
    auto renderer = app.node().make_child("BDPT").make_component<BDPT>();
    app->OnRenderWindow.add_listener(renderer.node(), [&](CommandBuffer& c) { renderer->render(c, W, H, {{view, view_xf}}, seeds); });
    const uint32_t rigs = for_each_mesh(*L.scene_node, set_rig);
    app->run_frame(cb);  // the first frame: a full upload of the rest poses; the rigs go up once behind it
    if (renderer->last_update_was_vertices_only() || renderer->last_update_was_transforms_only()) {
      std::printf("the first update cannot be a partial one\n");
      return 1;
    }
    if (!scene->pose_on_device() || scene->data()->mRigs.size() != rigs) return std::printf("the library has sthip_scene_animate: the scene must carry its rigs\n"), 1;
    for_each_mesh(*L.scene_node, set_pose);
    scene->mark_dirty();
    app->run_frame(cb);  // Scene::update repacks; BDPT::update: same geometry, same rigs, new poses
    const auto& fr = renderer->prev_result();
    std::ofstream out(argv[2], std::ios::binary);
    out.write((const char*)fr.mRadiance.data(), fr.mRadiance.size() * 4);
    out.write((const char*)fr.mPrevUVs.data(), fr.mPrevUVs.size() * 4);
    out.write((const char*)fr.mRayCount, 16);
    std::printf("ANIMATED vertices_only=%d transforms_only=%d rigs=%u\n", renderer->last_update_was_vertices_only() ? 1 : 0, renderer->last_update_was_transforms_only() ? 1 : 0, rigs);
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
