// environment_host.cpp — only the environment changes between two frames of the C++ host (stratum_amd/host/stratum_hip.hpp):
// the texels of the Environment's image are overwritten and Environment::mark_image_dirty() / set_value() are called, the scene
// is marked dirty, Scene::update repacks, and BDPT::update must find that nothing else changed and call
// sthip_scene_set_environment instead of uploading: last_update_was_environment_only(), and the call counts say so.
//   environment_host [--device-tables] [--host-only] [--move] <scene.bin> <sky.bin> <out.bin> <seeds>     (GPU)
// sky.bin: u32 H, u32 W, H*W*4 floats, the extent of the scene's environment image. The value becomes (0.5, 1.25, 2).
// --device-tables: the Environment is made with make_environment(..., tables_on_device = true) before the first frame.
// --host-only: Scene::set_environment_on_device(false), what a library without the symbol gets: the same change is an upload.
// --move: every node whose transform is not the identity moves by (0.25, 0.125, -0.25) in the frame the environment changes
// in: the environment is then not the only change, and the changed sky must still arrive (an upload). The graph that has the
// new environment from the start makes the same move between its two frames, so the motion transforms agree.
// A scene whose environment image a material also names makes the library refuse the call (unsupported): that is an upload too.
// A second scene graph is constructed with the new environment from the start and renders the same two frames; out.bin is the
// SECOND frame of the first graph (RGBA32F radiance, prev-uv, ray counts), and the program fails unless the second graph's
// second frame has the same bytes.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "../../stratum_amd/host/stratum_hip.hpp"
#include "scene_reader.hpp"

using namespace stm;

struct Sky {
  uint32_t h = 0, w = 0;
  std::vector<float> rgba;
};

struct Run {
  std::vector<float> radiance, prev_uv;
  uint64_t rays[2] = {0, 0};
  uint32_t uploads = 0, environment_calls = 0;
  bool environment_only = false;
};

// from_start: the new environment is in place before the first frame; otherwise it replaces the loaded one after it
static Run run(const char* scene_path, const Sky& sky, uint32_t seeds, bool device_tables, bool host_only, bool move, bool from_start) {
  Reader r(scene_path);
  NodeGraph graph;
  Node& root = graph.emplace("Instance");
  auto app = root.make_child("Application").make_component<Application>();
  LoadedScene L = load_scene(r, app.node());
  auto environment = L.scene_node->root().find_in_descendants<Environment>();
  if (!environment || !environment->image) throw std::runtime_error("the scene has no image environment");
  if (environment->image->width != sky.w || environment->image->height != sky.h) throw std::runtime_error("sky.bin has another extent than the scene's environment");
  if (host_only) L.scene->set_environment_on_device(false);
  if (device_tables) *environment = make_environment(environment->image, environment->value[0], environment->value[1], environment->value[2], true);
  const auto change = [&]() {
    environment->image->pixels = sky.rgba;
    environment->mark_image_dirty();
    environment->set_value(0.5f, 1.25f, 2.0f);
    L.scene->mark_dirty();
  };
  if (from_start) change();
  CommandBuffer cb;
  auto renderer = app.node().make_child("BDPT").make_component<BDPT>();
  app->OnRenderWindow.add_listener(renderer.node(), [&](CommandBuffer& c) { renderer->render(c, L.W, L.H, {{L.view, L.view_xf}}, seeds); });
  app->run_frame(cb);  // the first frame: a full upload
  if (renderer->last_update_was_environment_only()) throw std::runtime_error("the first update cannot be a partial one");
  if (!from_start) change();
  if (move) {
    L.scene_node->for_each_descendant<TransformData>([&](const component_ptr<TransformData>& t) {
      static const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
      if (std::memcmp(t.get(), I, sizeof(I)) == 0) return;
      t->m[0][3] += 0.25f;
      t->m[1][3] += 0.125f;
      t->m[2][3] -= 0.25f;
    });
    L.scene->mark_dirty();
  }
  app->run_frame(cb);
  const auto& fr = renderer->prev_result();
  Run out;
  out.radiance = fr.mRadiance;
  out.prev_uv = fr.mPrevUVs;
  std::memcpy(out.rays, fr.mRayCount, 16);
  out.uploads = renderer->upload_calls();
  out.environment_calls = renderer->environment_calls();
  out.environment_only = renderer->last_update_was_environment_only();
  return out;
}

int main(int argc, char** argv) {
  bool device_tables = false, host_only = false, move = false;
  int at = 1;
  for (; at < argc && argv[at][0] == '-'; at++) {
    if (!std::strcmp(argv[at], "--device-tables")) device_tables = true;
    else if (!std::strcmp(argv[at], "--host-only")) host_only = true;
    else if (!std::strcmp(argv[at], "--move")) move = true;
    else at = argc;
  }
  if (argc - at != 4) {
    std::fprintf(stderr, "usage: environment_host [--device-tables] [--host-only] [--move] scene.bin sky.bin out.bin seeds\n");
    return 2;
  }
  try {
    Sky sky;
    {
      std::ifstream f(argv[at + 1], std::ios::binary);
      uint32_t head[2] = {0, 0};
      f.read((char*)head, 8);
      sky.h = head[0], sky.w = head[1];
      sky.rgba.resize((size_t)sky.w * sky.h * 4);
      f.read((char*)sky.rgba.data(), sky.rgba.size() * 4);
      if (!f || !sky.w || !sky.h) return std::printf("cannot read %s\n", argv[at + 1]), 1;
    }
    const uint32_t seeds = (uint32_t)std::atoi(argv[at + 3]);
    const Run changed = run(argv[at], sky, seeds, device_tables, host_only, move, false);
    const Run fresh = run(argv[at], sky, seeds, device_tables, host_only, move, true);
    const bool same = changed.radiance.size() == fresh.radiance.size() && !std::memcmp(changed.radiance.data(), fresh.radiance.data(), fresh.radiance.size() * 4) &&
                      changed.prev_uv.size() == fresh.prev_uv.size() && !std::memcmp(changed.prev_uv.data(), fresh.prev_uv.data(), fresh.prev_uv.size() * 4) && !std::memcmp(changed.rays, fresh.rays, 16);
    std::ofstream out(argv[at + 2], std::ios::binary);
    out.write((const char*)changed.radiance.data(), changed.radiance.size() * 4);
    out.write((const char*)changed.prev_uv.data(), changed.prev_uv.size() * 4);
    out.write((const char*)changed.rays, 16);
    std::printf("ENVIRONMENT environment_only=%d uploads=%u environment_calls=%u same_as_from_start=%d fresh_uploads=%u fresh_environment_calls=%u\n", changed.environment_only ? 1 : 0, changed.uploads,
                changed.environment_calls, same ? 1 : 0, fresh.uploads, fresh.environment_calls);
    return same ? 0 : 1;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
