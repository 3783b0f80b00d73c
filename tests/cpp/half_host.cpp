// half_host.cpp — the C++ host with half colour precision on (BDPT::set_half_color_precision, the reference's
// mHalfColorPrecision): what Frame::mRadiance16 / mTonemapResult16 hold, export_hdr of a half frame, and the multi-GPU
// host's tile exchange with 8-byte entries.
//   half_host render <scene.bin> <out.bin> <seeds> <tonemap_mode> <exposure> <out.hdr>
//       BDPT, one frame: writes mRadiance16, mTonemapResult16 (RGBA16F bits) and the .hdr of export_hdr
//   half_host multi <scene.bin> <out.bin> <seeds> <devices>
//       MultiDeviceBDPT over `devices` (comma separated) in tile mode: writes mRadiance16, then checks that
//       split_seeds(true) is refused while the switch is on
#include <cstdio>
#include <fstream>
#include <sstream>

#include "../../stratum_amd/host/stratum_hip_multi.hpp"
#include "scene_reader.hpp"

using namespace stm;

static void write_u16(std::ofstream& out, const std::vector<uint16_t>& v) { out.write((const char*)v.data(), (std::streamsize)(v.size() * 2)); }

int main(int argc, char** argv) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: half_host render|multi scene.bin out.bin seeds ...\n");
    return 2;
  }
  try {
    const std::string mode = argv[1];
    Reader rd(argv[2]);
    NodeGraph graph;
    Node& root = graph.emplace("Instance");
    auto app = root.make_child("Application").make_component<Application>();
    LoadedScene L = load_scene(rd, app.node());
    const uint32_t seeds = (uint32_t)std::atoi(argv[4]);
    CommandBuffer cb;
    if (mode == "render" && argc >= 8) {
      auto renderer = app.node().make_child("BDPT").make_component<BDPT>();
      renderer->set_half_color_precision(true);
      renderer->tonemap_mode() = (uint32_t)std::atoi(argv[5]);
      renderer->exposure() = (float)std::atof(argv[6]);
      app->OnRenderWindow.add_listener(renderer.node(), [&](CommandBuffer& c) { renderer->render(c, L.W, L.H, {{L.view, L.view_xf}}, seeds); });
      app->run_frame(cb);
      const auto& fr = renderer->prev_result();
      const size_t n = (size_t)L.W * L.H * 4;
      if (fr.mRadiance16.size() != n || fr.mTonemapResult16.size() != n || fr.mAlbedo16.size() != n || !fr.mRadiance.empty() || !fr.mTonemapResult.empty()) {
        std::printf("FAIL: the half frame's images have the wrong sizes\n");
        return 1;
      }
      std::ofstream out(argv[3], std::ios::binary);
      write_u16(out, fr.mRadiance16);
      write_u16(out, fr.mTonemapResult16);
      renderer->export_hdr(argv[7]);
      std::printf("HALF RENDER OK %ux%u rays %llu\n", L.W, L.H, (unsigned long long)fr.mRayCount[0]);
      return 0;
    }
    if (mode == "multi" && argc >= 6) {
      std::vector<int> devices;
      std::stringstream ss(argv[5]);
      for (std::string tok; std::getline(ss, tok, ',');) devices.push_back(std::atoi(tok.c_str()));
      auto renderer = app.node().make_child("BDPT").make_component<MultiDeviceBDPT>(devices);
      renderer->set_half_color_precision(true);
      app->OnRenderWindow.add_listener(renderer.node(), [&](CommandBuffer& c) { renderer->render(c, L.W, L.H, {{L.view, L.view_xf}}, seeds); });
      app->run_frame(cb);
      const auto& fr = renderer->prev_result();
      if (fr.mRadiance16.size() != (size_t)L.W * L.H * 4 || !fr.mRadiance.empty()) {
        std::printf("FAIL: the half frame's radiance has the wrong size\n");
        return 1;
      }
      std::ofstream out(argv[3], std::ios::binary);
      write_u16(out, fr.mRadiance16);
      write_u16(out, fr.mAlbedo16);
      bool refused = false;
      try {
        renderer->split_seeds(true);
      } catch (const std::exception&) {
        refused = true;
      }
      std::printf("HALF MULTI OK world %zu, seed split %s\n", renderer->world(), refused ? "refused" : "ACCEPTED");
      return refused ? 0 : 1;
    }
    std::fprintf(stderr, "bad arguments\n");
    return 2;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
