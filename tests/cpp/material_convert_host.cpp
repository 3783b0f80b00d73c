// material_convert_host.cpp — the material conversions of the C++ host (stratum_amd/host/stratum_hip.hpp: Scene::
// make_metallic_roughness_material, make_diffuse_specular_material, shininess_to_roughness) with images, on the device.
//   material_convert_host <out.bin>   (GPU)
// The sources are 9 x 7 RGBA8 images whose bytes are a formula of (image, texel, channel) that tests/test_material_convert.py
// restates; the glTF material's alpha has one texel of 40 (alpha_test(): it keeps its mask), the diffuse/specular material's one
// of 200 (opaque: no mask). out.bin, per material: the 18 words of Material::store with resources of its own, min_alpha,
// has-mask, the three result images, the mask if it has one.
#include <cstdio>
#include <fstream>
#include <iostream>

#include "../../stratum_amd/host/stratum_hip.hpp"

using namespace stm;

static const uint32_t W = 9, H = 7;

static uint8_t texel_byte(uint32_t image, uint32_t i, uint32_t c) { return (uint8_t)((i * 37u + c * 101u + image * 59u + (i * i) % 251u) & 0xFFu); }

static component_ptr<Image> make_image(Node& parent, uint32_t image, int alpha_texel, uint8_t alpha) {
  auto im = parent.make_child("source").make_component<Image>();
  im->width = W, im->height = H;
  im->bytes.resize((size_t)W * H * 4);
  for (uint32_t i = 0; i < W * H; i++)
    for (uint32_t c = 0; c < 4; c++) im->bytes[i * 4 + c] = texel_byte(image, i, c);
  if (alpha_texel >= 0)
    for (uint32_t i = 0; i < W * H; i++) im->bytes[i * 4 + 3] = (int)i == alpha_texel ? alpha : 255;
  return im;
}

static void write_material(std::ofstream& out, const Material& m) {
  std::vector<uint32_t> words;
  MaterialResources resources;
  m.store(words, resources);
  out.write((const char*)words.data(), words.size() * 4);
  const uint32_t min_alpha = m.min_alpha, has_mask = m.alpha_mask ? 1 : 0;
  out.write((const char*)&min_alpha, 4);
  out.write((const char*)&has_mask, 4);
  for (int k = 0; k < 3; k++) out.write((const char*)m.values[k].image->bytes.data(), m.values[k].image->bytes.size());
  if (m.alpha_mask) out.write((const char*)m.alpha_mask->bytes.data(), m.alpha_mask->bytes.size());
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: material_convert_host out.bin\n");
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
    base_color.image = make_image(scene.node(), 0, 5, 40);
    metallic_roughness.value[1] = 0.3f, metallic_roughness.value[2] = 0.7f;
    metallic_roughness.image = make_image(scene.node(), 1, -1, 0);
    transmission.value[0] = 0.1f, transmission.value[1] = 0.2f, transmission.value[2] = 0.3f;
    transmission.image = make_image(scene.node(), 2, -1, 0);
    Material gltf = scene->make_metallic_roughness_material(cb, base_color, metallic_roughness, transmission, 1.4f, none3);
    if (!gltf.has_min_alpha || !gltf.alpha_test() || !gltf.alpha_mask) return std::printf("the glTF material must keep its alpha mask\n"), 1;

    ImageValue3 diffuse, specular;
    diffuse.value[0] = 0.6f, diffuse.value[1] = 0.5f, diffuse.value[2] = 0.4f;
    diffuse.image = make_image(scene.node(), 3, 3, 200);
    specular.value[0] = specular.value[1] = specular.value[2] = 0.2f;
    specular.image = make_image(scene.node(), 4, -1, 0);
    ImageValue1 shininess;
    shininess.value = 30.0f;
    shininess.image = scene.node().make_child("source").make_component<Image1>();
    shininess.image->width = W, shininess.image->height = H;
    shininess.image->bytes.resize((size_t)W * H);
    for (uint32_t i = 0; i < W * H; i++) shininess.image->bytes[i] = (uint8_t)((i * 11u + 7u) & 0xFFu);
    const ImageValue1 roughness = scene->shininess_to_roughness(cb, shininess);
    Material ds = scene->make_diffuse_specular_material(cb, diffuse, specular, roughness, transmission, 1.5f, none3);
    if (!ds.has_min_alpha || ds.alpha_test() || ds.alpha_mask) return std::printf("the diffuse/specular material is opaque: it must have no mask\n"), 1;

    std::ofstream out(argv[1], std::ios::binary);
    write_material(out, gltf);
    write_material(out, ds);
    out.write((const char*)&roughness.value, 4);
    out.write((const char*)roughness.image->bytes.data(), roughness.image->bytes.size());
    std::printf("CONVERTED min_alpha=%08x,%08x\n", gltf.min_alpha, ds.min_alpha);
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
