// top_level_host.cpp — instances move between frames of the C++ host (stratum_amd/host/stratum_hip.hpp) by each of its routes:
//   host            the nodes move twice; BDPT::update's transforms-only branch calls sthip_scene_update_transforms
//   device_builder  the same with Scene::set_top_level_on_device(true): the branch calls sthip_scene_set_transforms, top_level = 1
//   device_ptr      the nodes move once; the second move is made in device memory and handed over with
//                   BDPT::set_instance_transforms_device (inverse and motion derived by the library)
//   top_level_host <scene.bin> <out.bin> <seeds> <dx,dy,dz> <route>     (GPU)
// writes <out.bin>.f2 and <out.bin>.f3, the frames after the first and the second move: RGBA32F radiance, prev-uv, ray counts.
// Every node whose transform is not the identity moves by (dx, dy, dz) each time; the three routes must write the same bytes.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>

#include "../../stratum_amd/host/stratum_hip.hpp"
#include "scene_reader.hpp"

using namespace stm;

static bool is_identity(const void* t) {
  static const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  return std::memcmp(t, I, sizeof(I)) == 0;
}

int main(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: top_level_host scene.bin out.bin seeds dx,dy,dz host|device_builder|device_ptr\n");
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
    float dx = 0, dy = 0, dz = 0;
    std::sscanf(argv[4], "%f,%f,%f", &dx, &dy, &dz);
    const std::string route = argv[5];

    CommandBuffer cb;
    auto renderer = app.node().make_child("BDPT").make_component<BDPT>();
    app->OnRenderWindow.add_listener(renderer.node(), [&](CommandBuffer& c) { renderer->render(c, W, H, {{view, view_xf}}, seeds); });
    app->run_frame(cb);  // the first frame: a full upload
    auto move_nodes = [&]() {
      L.scene_node->for_each_descendant<TransformData>([&](const component_ptr<TransformData>& t) {
        if (is_identity(t.get())) return;
        t->m[0][3] += dx;
        t->m[1][3] += dy;
        t->m[2][3] += dz;
      });
      scene->mark_dirty();
    };
    auto write = [&](const char* suffix) {
      const auto& fr = renderer->prev_result();
      std::ofstream out(std::string(argv[2]) + suffix, std::ios::binary);
      out.write((const char*)fr.mRadiance.data(), fr.mRadiance.size() * 4);
      out.write((const char*)fr.mPrevUVs.data(), fr.mPrevUVs.size() * 4);
      out.write((const char*)fr.mRayCount, 16);
    };
    if (route == "device_builder") scene->set_top_level_on_device(true);
    move_nodes();
    app->run_frame(cb);
    const bool first_was_transforms_only = renderer->last_update_was_transforms_only();
    write(".f2");
    if (route == "device_ptr") {
      std::vector<TransformData> xf = scene->data()->mInstanceTransforms;
      for (TransformData& t : xf) {
        if (is_identity(&t)) continue;
        t.m[0][3] += dx;
        t.m[1][3] += dy;
        t.m[2][3] += dz;
      }
      void* d = nullptr;
      if (hipMalloc(&d, xf.size() * sizeof(TransformData)) != hipSuccess || hipMemcpy(d, xf.data(), xf.size() * sizeof(TransformData), hipMemcpyHostToDevice) != hipSuccess) {
        std::printf("hipMalloc / hipMemcpy failed\n");
        return 1;
      }
      renderer->set_instance_transforms_device(d, nullptr, nullptr, true);
      (void)hipFree(d);  // (the call has finished with the array when it returns)
    } else {
      move_nodes();
    }
    app->run_frame(cb);
    write(".f3");
    std::printf("MOVED route=%s transforms_only=%d on_device=%d\n", route.c_str(), first_was_transforms_only ? 1 : 0, scene->top_level_on_device() ? 1 : 0);
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
