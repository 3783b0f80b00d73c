// multi_deform_mock.cpp — a mesh deforms under stm::MultiDeviceBDPT, over the stand-ins of multi_mock.cpp (no GPU). The
// driver's ranks must all walk the same tree form, and it sends them uploads or transforms-only updates: BDPT::update's
// vertices-only refit is switched off for it (mRefitDeformedMeshes), so rank 0 must not refit while the others upload.
// This file adds a stand-in for sthip_scene_update_vertices that counts its calls: it must never be called, and
// last_update_was_vertices_only() must stay false.
//   multi_deform_mock <scene.bin> <world>
#define main multi_mock_main
#include "multi_mock.cpp"
#undef main

#include <unordered_set>

namespace mock {
std::atomic<int> vertex_updates{0};
}
extern "C" int sthip_scene_update_vertices(sthip_ctx*, const sthip_PackedVertexData*, uint32_t, uint32_t, sthip_refit_info*) {
  mock::vertex_updates++;
  return STHIP_OK;
}

int main(int argc, char** argv) {
  if (argc < 3) return std::fprintf(stderr, "usage: multi_deform_mock scene.bin world\n"), 2;
  alarm(120);
  try {
    const int world = atoi(argv[2]);
    std::vector<int> devices;
    for (int r = 0; r < world; r++) devices.push_back(r);
    Reader rd(argv[1]);
    NodeGraph graph;
    Node& root = graph.emplace("Instance");
    auto app = root.make_child("Application").make_component<Application>();
    LoadedScene L = load_scene(rd, app.node());
    auto renderer = app.node().make_child("BDPT").make_component<MultiDeviceBDPT>(devices, 64, 32);
    app->OnRenderWindow.add_listener(renderer.node(), [&](CommandBuffer& c) { renderer->render(c, L.W, L.H, {{L.view, L.view_xf}}, 1); });
    CommandBuffer cb;
    app->run_frame(cb);
    if (check_frame(renderer->prev_result(), L.W, L.H, 0, true, "first frame")) return 1;
    std::unordered_set<const Mesh*> done;
    uint32_t edits = 0;
    L.scene_node->root().for_each_descendant<MeshPrimitive>([&](const component_ptr<MeshPrimitive>& prim) {
      if (!prim->mMesh || !done.insert(prim->mMesh.get()).second) return;
      auto p = prim->mMesh->positions;
      for (auto& q : p) q.y = q.y + 0.04f * (q.x * q.z);
      prim->set_vertices(std::move(p));
      edits++;
    });
    if (!edits) return std::printf("FAIL: no mesh to deform\n"), 1;
    L.scene->mark_dirty();
    app->run_frame(cb);
    if (check_frame(renderer->prev_result(), L.W, L.H, 1, true, "after the deformation")) return 1;
    if (mock::vertex_updates.load() != 0) return std::printf("FAIL: sthip_scene_update_vertices was called %d times under the multi-device driver\n", mock::vertex_updates.load()), 1;
    if (renderer->last_update_was_vertices_only() || renderer->last_update_was_transforms_only()) return std::printf("FAIL: the deformation was not a full upload\n"), 1;
    std::printf("MULTI DEFORM OK world %d meshes %u\n", world, edits);
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
