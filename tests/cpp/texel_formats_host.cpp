// texel_formats_host.cpp — images in an asset's own texel format through the C++ host (stratum_amd/host/stratum_hip.hpp: Image::
// texels / texel_format, Scene::make_metallic_roughness_material, Scene::decode_image), on the device.
//   texel_formats_host <out.bin>   (GPU)
// The sources are 9 x 7 images whose bytes are a formula of (image, byte index) that tests/test_texel_formats.py restates: a glTF
// material from an RGBA8_SRGB base colour (one texel of alpha 40: it keeps its mask) and an RGB8_UNORM metallic/roughness image,
// with an RGB8_UNORM normal map bound as bump_image; and an emissive material whose RGBA8_SRGB emission image becomes its base
// colour image. out.bin: for the glTF material the 18 words of Material::store with resources of its own, min_alpha, the three
// result images, the mask and the bump image (bytes); for the emissive one the 18 words and the base colour image (binary32).
#include <cstdio>
#include <fstream>
#include <iostream>

#include "../../stratum_amd/host/stratum_hip.hpp"

using namespace stm;

static const uint32_t W = 9, H = 7;

static component_ptr<Image> make_raw(Node& parent, uint32_t image, uint32_t format, uint32_t channels, int alpha_texel, uint8_t alpha) {
  auto im = parent.make_child("source").make_component<Image>();
  im->width = W, im->height = H;
  im->texel_format = format;
  im->texels.resize((size_t)W * H * channels);
  for (uint32_t i = 0; i < im->texels.size(); i++) im->texels[i] = (uint8_t)((i * 29u + image * 71u + (i * i) % 241u) & 0xFFu);
  if (alpha_texel >= 0)
    for (uint32_t i = 0; i < W * H; i++) im->texels[i * 4 + 3] = (int)i == alpha_texel ? alpha : 255;
  return im;
}

static void write_words(std::ofstream& out, const Material& m) {
  std::vector<uint32_t> words;
  MaterialResources resources;
  m.store(words, resources);
  out.write((const char*)words.data(), words.size() * 4);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: texel_formats_host out.bin\n");
    return 2;
  }
  try {
    NodeGraph graph;
    Node& root = graph.emplace("Instance");
    auto app = root.make_child("Application").make_component<Application>();
    auto scene = app.node().make_child("Scene").make_component<Scene>();
    auto renderer = app.node().make_child("BDPT").make_component<BDPT>();
    CommandBuffer cb;
    cb.ctx = renderer->context();

    ImageValue3 base_color, transmission, none3;
    ImageValue4 metallic_roughness;
    base_color.value[0] = 0.5f, base_color.value[1] = 0.25f, base_color.value[2] = 0.75f;
    base_color.image = make_raw(scene.node(), 0, STHIP_TEXEL_RGBA8_SRGB, 4, 5, 40);
    metallic_roughness.value[1] = 0.3f, metallic_roughness.value[2] = 0.7f;
    metallic_roughness.image = make_raw(scene.node(), 1, STHIP_TEXEL_RGB8_UNORM, 3, -1, 0);
    Material gltf = scene->make_metallic_roughness_material(cb, base_color, metallic_roughness, transmission, 1.4f, none3);
    if (!gltf.has_min_alpha || !gltf.alpha_test() || !gltf.alpha_mask) return std::printf("the glTF material must keep its alpha mask\n"), 1;
    gltf.bump_image = scene->decode_image(cb, *make_raw(scene.node(), 2, STHIP_TEXEL_RGB8_UNORM, 3, -1, 0));
    if (!gltf.bump_image->is_8bit() || gltf.bump_image->is_raw()) return std::printf("an RGB8 normal map decodes to its bytes: the image stays 8-bit\n"), 1;

    ImageValue3 emission;
    emission.value[0] = 2.0f, emission.value[1] = 1.5f, emission.value[2] = 1.0f;
    emission.image = make_raw(scene.node(), 3, STHIP_TEXEL_RGBA8_SRGB, 4, -1, 0);
    Material light = scene->make_metallic_roughness_material(cb, none3, metallic_roughness, transmission, 1.4f, emission);
    if (!light.values[0].image || light.values[0].image->is_raw() || light.values[0].image->is_8bit()) return std::printf("an sRGB emission image decodes to binary32\n"), 1;

    std::ofstream out(argv[1], std::ios::binary);
    write_words(out, gltf);
    out.write((const char*)&gltf.min_alpha, 4);
    for (int k = 0; k < 3; k++) out.write((const char*)gltf.values[k].image->bytes.data(), gltf.values[k].image->bytes.size());
    out.write((const char*)gltf.alpha_mask->bytes.data(), gltf.alpha_mask->bytes.size());
    out.write((const char*)gltf.bump_image->bytes.data(), gltf.bump_image->bytes.size());
    write_words(out, light);
    out.write((const char*)light.values[0].image->pixels.data(), light.values[0].image->pixels.size() * 4);
    std::printf("DECODED min_alpha=%08x\n", gltf.min_alpha);
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
