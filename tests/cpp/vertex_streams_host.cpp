// vertex_streams_host.cpp — a mesh deforms between frames of the C++ host (stratum_amd/host/stratum_hip.hpp) by each of its
// routes, three hosts in one process, three frames each (a frame's seed is its number, so frames are compared by number):
//   update   frame 2 after MeshPrimitive::set_vertices + mark_dirty (BDPT::update: the host vertex call), frame 3 after the
//            rest positions were set again the same way
//   device   frame 2 after BDPT::set_vertices_device from a hipMalloc'd copy of the deformed records (positions at a stride
//            of 32 bytes; normals and uvs stay), frame 3 after mark_dirty alone: the scene graph still holds the rest
//            positions, so BDPT::update must send them — it must not take the bound data's vertices for the resident ones
//   fresh    a host whose meshes are deformed before its first frame: an upload
// Frame 2 must be the same bytes by all three routes, frame 3 by the first two (and not the fresh host's, which stays deformed).
//   vertex_streams_host <scene.bin>     (GPU) prints one line per comparison and "VERTEX STREAMS HOST OK"
// The displacement is y += 0.04 * (x * z), as in deform_host.cpp.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../stratum_amd/host/stratum_hip.hpp"
#include "scene_reader.hpp"

using namespace stm;

static void displace(float& x, float& y, float& z) {
  const float xz = x * z;
  const float d = 0.04f * xz;
  y = y + d;
}

template <typename F>
static void for_each_mesh(Node& scene_node, F&& f) {  // every mesh once (instances may share one), through the primitive that carries it
  std::unordered_set<const Mesh*> done;
  scene_node.root().for_each_descendant<MeshPrimitive>([&](const component_ptr<MeshPrimitive>& prim) {
    if (!prim->mMesh || !done.insert(prim->mMesh.get()).second) return;
    f(*prim);
  });
}

struct Frames {
  std::vector<uint8_t> f[3];
  uint32_t uploads = 0;
  bool vertices_only[3] = {false, false, false};
};

static std::vector<uint8_t> bytes_of(const BDPT::Frame& fr) {
  std::vector<uint8_t> out(fr.mRadiance.size() * 4 + fr.mPrevUVs.size() * 4 + 16);
  std::memcpy(out.data(), fr.mRadiance.data(), fr.mRadiance.size() * 4);
  std::memcpy(out.data() + fr.mRadiance.size() * 4, fr.mPrevUVs.data(), fr.mPrevUVs.size() * 4);
  std::memcpy(out.data() + out.size() - 16, fr.mRayCount, 16);
  return out;
}

static Frames run(const char* path, const std::string& route) {
  Reader r(path);
  NodeGraph graph;
  Node& root = graph.emplace("Instance");
  auto app = root.make_child("Application").make_component<Application>();
  LoadedScene L = load_scene(r, app.node());
  auto scene = L.scene;
  const ViewData view = L.view;
  const TransformData view_xf = L.view_xf;
  const uint32_t W = L.W, H = L.H;
  CommandBuffer cb;
  auto renderer = app.node().make_child("BDPT").make_component<BDPT>();
  app->OnRenderWindow.add_listener(renderer.node(), [&](CommandBuffer& c) { renderer->render(c, W, H, {{view, view_xf}}, 1); });
  Frames out;
  std::vector<std::pair<MeshPrimitive*, std::vector<stm::float3>>> rest;
  for_each_mesh(*L.scene_node, [&](MeshPrimitive& prim) { rest.emplace_back(&prim, prim.mMesh->positions); });
  auto deform = [&]() {
    for (auto& m : rest) {
      std::vector<stm::float3> p = m.second;
      for (stm::float3& q : p) displace(q.x, q.y, q.z);
      m.first->set_vertices(std::move(p));
    }
    scene->mark_dirty();
  };
  auto frame = [&](int k) {
    app->run_frame(cb);
    out.f[k] = bytes_of(renderer->prev_result());
    out.vertices_only[k] = renderer->last_update_was_vertices_only();
  };
  if (route == "fresh") deform();
  frame(0);
  if (route == "update") {
    deform();
  } else if (route == "device") {
    // the deformed records, made from the packed ones as the graph's route makes them from the meshes' positions
    std::vector<float> records(scene->data()->mVertices.size() * 8);
    static_assert(sizeof(scene->data()->mVertices[0]) == 32, "PackedVertexData");
    std::memcpy(records.data(), scene->data()->mVertices.data(), records.size() * 4);
    for (size_t i = 0; i < records.size(); i += 8) displace(records[i], records[i + 1], records[i + 2]);
    void* d = nullptr;
    if (hipMalloc(&d, records.size() * 4) != hipSuccess || hipMemcpy(d, records.data(), records.size() * 4, hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("hipMalloc / hipMemcpy failed");
    sthip_refit_info info{};
    renderer->set_vertices_device(0, (uint32_t)(records.size() / 8), d, 32, nullptr, 0, nullptr, 0, false, &info);
    (void)hipFree(d);  // (the call has finished with the stream when it returns)
    if (!renderer->vertices_behind_device()) throw std::runtime_error("the bound vertices are not marked as behind the device");
  }
  frame(1);
  if (route == "update") {
    for (auto& m : rest) m.first->set_vertices(m.second);
    scene->mark_dirty();
  } else if (route == "device") {
    scene->mark_dirty();  // (nothing of the graph changed: it still holds the rest positions)
  }
  frame(2);
  out.uploads = renderer->upload_calls();
  return out;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: vertex_streams_host scene.bin\n");
    return 2;
  }
  try {
    const Frames update = run(argv[1], "update"), device = run(argv[1], "device"), fresh = run(argv[1], "fresh");
    int failures = 0;
    auto check = [&](const char* what, bool ok) {
      std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
      if (!ok) failures++;
    };
    check("frame 1 is the same on the update and the device host", update.f[0] == device.f[0] && !update.f[0].empty());
    check("the deformation changes frame 1 of the fresh host", fresh.f[0] != update.f[0]);
    check("update: the deformation went through the host vertex call", update.vertices_only[1] && update.uploads == 1);
    check("frame 2: set_vertices_device equals BDPT::update", device.f[1] == update.f[1]);
    check("frame 2: a fresh host equals BDPT::update", fresh.f[1] == update.f[1]);
    check("frame 3: the deformation would show", fresh.f[2] != update.f[2]);
    check("frame 3: an update after the device call sends the graph's vertices", device.f[2] == update.f[2]);
    check("device: that update was an upload", device.uploads == 2 && !device.vertices_only[2]);
    if (failures) return std::printf("%d FAILED\n", failures), 1;
    std::printf("VERTEX STREAMS HOST OK\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
