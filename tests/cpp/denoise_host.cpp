// denoise_host.cpp — the C++ host (stratum_amd/host/stratum_hip.hpp) with a Denoiser component beside BDPT, as Stratum's
// main.cpp makes one (BDPT.cpp:472-473,767-781): N frames of one sample each through Application::run_frame, the last
// frame's tone-mapped image written as RGBA32F.
//   denoise_host <scene.bin> <out.bin> <frames> <tonemap_mode> <exposure> <denoiser 0|1> [iterations filter_type history_tap
//                history_limit variance_boost_length]   (GPU)
#include <cstdio>
#include <fstream>

#include "../../stratum_amd/host/stratum_hip.hpp"
#include "scene_reader.hpp"

using namespace stm;

int main(int argc, char** argv) {
  if (argc < 7) {
    std::fprintf(stderr, "usage: denoise_host scene.bin out.bin frames tonemap_mode exposure denoiser [iterations filter_type history_tap history_limit variance_boost_length]\n");
    return 2;
  }
  try {
    Reader r(argv[1]);
    NodeGraph graph;
    Node& root = graph.emplace("Instance");
    auto app = root.make_child("Application").make_component<Application>();
    LoadedScene L = load_scene(r, app.node());
    const ViewData view = L.view;
    const TransformData view_xf = L.view_xf;
    const uint32_t W = L.W, H = L.H;
    const int frames = std::atoi(argv[3]);
    auto renderer = app.node().make_child("BDPT").make_component<BDPT>();
    renderer->tonemap_mode() = (uint32_t)std::atoi(argv[4]);
    renderer->exposure() = (float)std::atof(argv[5]);
    if (std::atoi(argv[6])) {
      auto denoiser = renderer.node().make_component<Denoiser>();
      if (argc >= 12) {
        denoiser->atrous_iterations() = (uint32_t)std::atoi(argv[7]);
        denoiser->filter_type() = (uint32_t)std::atoi(argv[8]);
        denoiser->history_tap() = (uint32_t)std::atoi(argv[9]);
        denoiser->history_limit() = (float)std::atof(argv[10]);
        denoiser->variance_boost_length() = (float)std::atof(argv[11]);
      }
    }
    CommandBuffer cb;
    app->OnRenderWindow.add_listener(renderer.node(), [&](CommandBuffer& c) { renderer->render(c, W, H, {{view, view_xf}}, 1); });
    for (int i = 0; i < frames; i++) app->run_frame(cb);
    const auto& fr = renderer->prev_result();
    std::ofstream out(argv[2], std::ios::binary);
    out.write((const char*)fr.mTonemapResult.data(), fr.mTonemapResult.size() * 4);
    std::printf("DENOISE HOST OK %ux%u frames %d denoised %d\n", W, H, frames, fr.mDenoiseResult.empty() ? 0 : 1);
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
