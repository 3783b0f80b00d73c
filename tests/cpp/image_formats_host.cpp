// image_formats_host.cpp — 8-bit textures through the C++ host (stratum_amd/host/stratum_hip.hpp): the scene description
// carries float images whose texels are all k / 255; every Image and Image1 is turned into its bytes (Image::bytes,
// Image1::bytes) before the first Scene::update, which must then hand the bytes over with format 1 and
// BDPT::update must upload them through sthip_scene_upload_formats.
//   image_formats_host pack   <scene.bin>                  (no GPU) what Scene::update packed: formats and descriptors
//   image_formats_host render <scene.bin> <out.bin> <seeds> (GPU) RGBA32F radiance and the ray counts of one frame
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>

#include "../../stratum_amd/host/stratum_hip.hpp"
#include "scene_reader.hpp"

using namespace stm;

template <typename T>
static bool to_bytes(T& im) {
  im.bytes.resize(im.pixels.size());
  for (size_t i = 0; i < im.pixels.size(); i++) {
    const long b = std::lrintf(im.pixels[i] * 255.0f);
    if (b < 0 || b > 255 || (float)b / 255.0f != im.pixels[i]) return false;  // (not a decoded byte: the description is wrong)
    im.bytes[i] = (uint8_t)b;
  }
  im.pixels.clear();
  return true;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: image_formats_host pack|render scene.bin [out.bin seeds]\n");
    return 2;
  }
  try {
    const std::string mode = argv[1];
    Reader r(argv[2]);
    NodeGraph graph;
    Node& root = graph.emplace("Instance");
    auto app = root.make_child("Application").make_component<Application>();
    LoadedScene L = load_scene(r, app.node());
    bool ok = true;
    uint32_t converted = 0;
    L.scene_node->for_each_descendant<Image>([&](const component_ptr<Image>& im) { ok = to_bytes(*im) && ok, converted++; });
    L.scene_node->for_each_descendant<Image1>([&](const component_ptr<Image1>& im) { ok = to_bytes(*im) && ok, converted++; });
    if (!ok) {
      std::printf("a texel of the description is not k / 255\n");
      return 1;
    }
    CommandBuffer cb;
    if (mode == "pack") {
      L.scene->update(cb, 0);
      const auto& sd = *L.scene->data();
      uint32_t as_bytes = 0;
      for (size_t i = 0; i < sd.mImageDescs.size(); i++) {
        const Image* im = sd.mResources.image4s[i];
        if (sd.mImageFormats[i] == STHIP_IMAGE_FORMAT_RGBA8_UNORM && (const void*)sd.mImageDescs[i].pixels == (const void*)im->bytes.data()) as_bytes++;
      }
      for (size_t i = 0; i < sd.mImage1Descs.size(); i++) {
        const Image1* im = sd.mResources.image1s[i];
        if (sd.mImage1Formats[i] == STHIP_IMAGE_FORMAT_R8_UNORM && (const void*)sd.mImage1Descs[i].pixels == (const void*)im->bytes.data()) as_bytes++;
      }
      std::printf("PACKED converted=%u images=%zu masks=%zu as_bytes=%u host_floats=%zu\n", converted, sd.mImageDescs.size(), sd.mImage1Descs.size(), as_bytes, sd.mConvertedImages.size());
      return 0;
    }
    if (argc < 5) return 2;
    const ViewData view = L.view;
    const TransformData view_xf = L.view_xf;
    const uint32_t W = L.W, H = L.H, seeds = (uint32_t)std::atoi(argv[4]);
    auto renderer = app.node().make_child("BDPT").make_component<BDPT>();
    app->OnRenderWindow.add_listener(renderer.node(), [&](CommandBuffer& c) { renderer->render(c, W, H, {{view, view_xf}}, seeds); });
    app->run_frame(cb);
    const auto& fr = renderer->prev_result();
    std::ofstream out(argv[3], std::ios::binary);
    out.write((const char*)fr.mRadiance.data(), fr.mRadiance.size() * 4);
    out.write((const char*)fr.mRayCount, 16);
    std::printf("RENDERED converted=%u\n", converted);
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
