// volume_host.cpp — only a medium's density grid changes between two frames of the C++ host (stratum_amd/host/stratum_hip.hpp):
// Medium::set_density_device() names a dense box in device memory, the scene is marked dirty, Scene::update repacks, and
// BDPT::update must find that nothing else changed and call sthip_scene_set_volume instead of uploading:
// last_update_was_volumes_only(), and the call counts say so.
//   volume_host [--host-only] <scene.bin> <dense.bin> <out.bin> <seeds>     (GPU)
// dense.bin: u32 dims[3], i32 origin[3], f64 voxel_size, f64 translation[3], then dims[0]*dims[1]*dims[2] floats.
// --host-only: BDPT::set_volumes_on_device(false), what a library without the symbol gets: the grid is built into the host's
// buffer (sthip_build_volume) and the same change is an upload.
// A second scene graph has the dense source from the start (its first upload builds the grid) and renders the same two
// frames; out.bin is the SECOND frame of the first graph (RGBA32F radiance, prev-uv, ray counts), and the program fails
// unless the second graph's second frame has the same bytes.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "../../stratum_amd/host/stratum_hip.hpp"
#include "scene_reader.hpp"

using namespace stm;

struct Dense {
  uint32_t dims[3] = {0, 0, 0};
  int32_t origin[3] = {0, 0, 0};
  double voxel_size = 1, translation[3] = {0, 0, 0};
  std::vector<float> values;
  float* device = nullptr;
};

struct Run {
  std::vector<float> radiance, prev_uv;
  uint64_t rays[2] = {0, 0};
  uint32_t uploads = 0, volume_calls = 0;
  bool volumes_only = false;
};

// from_start: the dense source is in place before the first frame; otherwise it replaces the loaded grid after it
static Run run(const char* scene_path, const Dense& dense, uint32_t seeds, bool host_only, bool from_start) {
  Reader r(scene_path);
  NodeGraph graph;
  Node& root = graph.emplace("Instance");
  auto app = root.make_child("Application").make_component<Application>();
  LoadedScene L = load_scene(r, app.node());
  auto medium = L.scene_node->root().find_in_descendants<Medium>();
  if (!medium || !medium->density_buffer) throw std::runtime_error("the scene has no medium");
  const auto change = [&]() {
    medium->set_density_device(dense.device, dense.dims, dense.origin, dense.voxel_size, dense.translation, "density");
    L.scene->mark_dirty();
  };
  if (from_start) change();
  CommandBuffer cb;
  auto renderer = app.node().make_child("BDPT").make_component<BDPT>();
  if (host_only) renderer->set_volumes_on_device(false);
  app->OnRenderWindow.add_listener(renderer.node(), [&](CommandBuffer& c) { renderer->render(c, L.W, L.H, {{L.view, L.view_xf}}, seeds); });
  app->run_frame(cb);  // the first frame: a full upload
  if (renderer->last_update_was_volumes_only()) throw std::runtime_error("the first update cannot be a partial one");
  if (!from_start) change();
  app->run_frame(cb);
  const auto& fr = renderer->prev_result();
  Run out;
  out.radiance = fr.mRadiance;
  out.prev_uv = fr.mPrevUVs;
  std::memcpy(out.rays, fr.mRayCount, 16);
  out.uploads = renderer->upload_calls();
  out.volume_calls = renderer->volume_calls();
  out.volumes_only = renderer->last_update_was_volumes_only();
  double box[6];
  if (!medium->world_bbox(box) || !(box[0] < box[3])) throw std::runtime_error("the medium has no world box");
  return out;
}

int main(int argc, char** argv) {
  bool host_only = false;
  int at = 1;
  for (; at < argc && argv[at][0] == '-'; at++) {
    if (!std::strcmp(argv[at], "--host-only")) host_only = true;
    else at = argc;
  }
  if (argc - at != 4) {
    std::fprintf(stderr, "usage: volume_host [--host-only] scene.bin dense.bin out.bin seeds\n");
    return 2;
  }
  try {
    Dense dense;
    {
      std::ifstream f(argv[at + 1], std::ios::binary);
      f.read((char*)dense.dims, 12);
      f.read((char*)dense.origin, 12);
      f.read((char*)&dense.voxel_size, 8);
      f.read((char*)dense.translation, 24);
      dense.values.resize((size_t)dense.dims[0] * dense.dims[1] * dense.dims[2]);
      f.read((char*)dense.values.data(), dense.values.size() * 4);
      if (!f || dense.values.empty()) return std::printf("cannot read %s\n", argv[at + 1]), 1;
    }
    if (hipMalloc((void**)&dense.device, dense.values.size() * 4) != hipSuccess || hipMemcpy(dense.device, dense.values.data(), dense.values.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
      return std::printf("no device memory for the dense box\n"), 1;
    const uint32_t seeds = (uint32_t)std::atoi(argv[at + 3]);
    const Run changed = run(argv[at], dense, seeds, host_only, false);
    const Run fresh = run(argv[at], dense, seeds, host_only, true);
    (void)hipFree(dense.device);
    const bool same = changed.radiance.size() == fresh.radiance.size() && !std::memcmp(changed.radiance.data(), fresh.radiance.data(), fresh.radiance.size() * 4) &&
                      changed.prev_uv.size() == fresh.prev_uv.size() && !std::memcmp(changed.prev_uv.data(), fresh.prev_uv.data(), fresh.prev_uv.size() * 4) && !std::memcmp(changed.rays, fresh.rays, 16);
    std::ofstream out(argv[at + 2], std::ios::binary);
    out.write((const char*)changed.radiance.data(), changed.radiance.size() * 4);
    out.write((const char*)changed.prev_uv.data(), changed.prev_uv.size() * 4);
    out.write((const char*)changed.rays, 16);
    std::printf("VOLUME volumes_only=%d uploads=%u volume_calls=%u same_as_from_start=%d fresh_uploads=%u fresh_volume_calls=%u\n", changed.volumes_only ? 1 : 0, changed.uploads, changed.volume_calls, same ? 1 : 0,
                fresh.uploads, fresh.volume_calls);
    return same ? 0 : 1;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
