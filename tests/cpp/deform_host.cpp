// deform_host.cpp — a mesh deforms between two frames of the C++ host (stratum_amd/host/stratum_hip.hpp): every
// MeshPrimitive gets new vertex positions through MeshPrimitive::set_vertices, the scene is marked dirty, Scene::update
// repacks, and BDPT::update must find that only vertex contents changed and refit (sthip_scene_update_vertices) instead
// of uploading: last_update_was_vertices_only().
//   deform_host <scene.bin> <out.bin> <seeds>     (GPU) writes the SECOND frame: RGBA32F radiance, prev-uv, ray counts
// The displacement is y += 0.04 * (x * z), three binary32 roundings a numpy host reproduces exactly.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <unordered_set>

#include "../../stratum_amd/host/stratum_hip.hpp"
#include "scene_reader.hpp"

using namespace stm;

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: deform_host scene.bin out.bin seeds\n");
    return 2;
  }
  try {
    Reader r(argv[1]);
    NodeGraph graph;
    Node& root = graph.emplace("Instance");
    auto app = root.make_child("Application").make_component<Application>();
    LoadedScene L = load_scene(r, app.node());
    auto scene = L.scene;
    const ViewData view = L.view;
    const TransformData view_xf = L.view_xf;
    const uint32_t W = L.W, H = L.H;
    const uint32_t seeds = (uint32_t)std::atoi(argv[3]);

    CommandBuffer cb;
    auto renderer = app.node().make_child("BDPT").make_component<BDPT>();
    app->OnRenderWindow.add_listener(renderer.node(), [&](CommandBuffer& c) { renderer->render(c, W, H, {{view, view_xf}}, seeds); });
    app->run_frame(cb);  // the first frame: a full upload
    if (renderer->last_update_was_vertices_only() || renderer->last_update_was_transforms_only()) {
      std::printf("the first update cannot be a partial one\n");
      return 1;
    }
    // every mesh once (instances may share one), through the primitive that carries it
    std::unordered_set<const Mesh*> done;
    uint32_t edits = 0;
    L.scene_node->root().for_each_descendant<MeshPrimitive>([&](const component_ptr<MeshPrimitive>& prim) {
      if (!prim->mMesh || !done.insert(prim->mMesh.get()).second) return;
      std::vector<float3> p = prim->mMesh->positions;
      for (float3& q : p) {
        const float xz = q.x * q.z;
        const float d = 0.04f * xz;
        q.y = q.y + d;
      }
      prim->set_vertices(std::move(p));
      edits++;
    });
    scene->mark_dirty();
    app->run_frame(cb);  // Scene::update repacks; BDPT::update: same topology, new vertex contents
    const auto& fr = renderer->prev_result();
    std::ofstream out(argv[2], std::ios::binary);
    out.write((const char*)fr.mRadiance.data(), fr.mRadiance.size() * 4);
    out.write((const char*)fr.mPrevUVs.data(), fr.mPrevUVs.size() * 4);
    out.write((const char*)fr.mRayCount, 16);
    std::printf("DEFORMED vertices_only=%d transforms_only=%d meshes=%u\n", renderer->last_update_was_vertices_only() ? 1 : 0, renderer->last_update_was_transforms_only() ? 1 : 0, edits);
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
