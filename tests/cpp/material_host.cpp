// material_host.cpp — which path BDPT::update of the C++ host (stratum_amd/host/stratum_hip.hpp) takes when only materials
// change between two frames, WITHOUT a GPU: the C ABI is replaced by stand-ins defined in this file. The stand-ins keep what an
// upload would keep on the host and decide the two material calls with the library's own host checks
// (stratum_amd/csrc/scene_prepare.cpp: check_images, check_material_data), so a refusal here is a refusal there.
//   material_host <scene.bin> <mode>
// mode colour : the base colour of the first material changes                -> sthip_scene_set_material_data, no upload
//      texture: the texels of the first image are repainted + mark_dirty()   -> sthip_scene_set_images, no upload
//      both   : both of the above                                            -> one call each, no upload
//      extent : the first image gets another extent + mark_dirty()           -> upload
//      emitter: the first emissive material stops emitting (the light list changes with it) -> upload
//      off    : colour, with a BDPT whose mMaterialsOnDevice is false        -> upload
// Prints one line "MATERIALS ..." with the path and the counters.
#include <cstdio>
#include <cstring>
#include <iostream>

#include "../../stratum_amd/csrc/scene_prepare.h"
#include "../../stratum_amd/host/stratum_hip.hpp"
#include "scene_reader.hpp"

using namespace stm;

// ------------------------------------------------------------------ the stand-ins ------------------------------------------------------------------
struct sthip_ctx {
  std::string error;
  bool has_scene = false;
  std::vector<uint8_t> materials;
  std::vector<sthip::MaterialInstance> instances;
  std::vector<DeviceImage> images;
  std::vector<DeviceImage1> images1;
  uint32_t volume_count = 0;
  uint32_t uploads = 0, data_calls = 0, image_calls = 0, data_offset = 0, data_bytes = 0, images_sent = 0, refused = 0;
};
static sthip_ctx* g_ctx = nullptr;

static int keep_scene(sthip_ctx* c, const sthip_scene_desc* s, const uint8_t* formats, const uint8_t* formats1) {
  c->uploads++;
  c->has_scene = true;
  c->materials.assign((const uint8_t*)s->gMaterialData, (const uint8_t*)s->gMaterialData + s->material_bytes);
  c->instances.clear();
  for (uint32_t i = 0; i < s->instance_count; i++) c->instances.push_back(sthip::MaterialInstance{s->gInstances[i].packed[0] >> 4, s->gInstances[i].packed[0] & 0xFu});
  c->images.assign(s->image_count, DeviceImage{});
  for (uint32_t i = 0; i < s->image_count; i++) {
    c->images[i].w[0] = (uint16_t)s->gImages[i].width, c->images[i].h[0] = (uint16_t)s->gImages[i].height;
    c->images[i].levels = 1, c->images[i].format = formats ? formats[i] : 0;
  }
  c->images1.assign(s->image1_count, DeviceImage1{});
  for (uint32_t i = 0; i < s->image1_count; i++) c->images1[i] = DeviceImage1{0, s->gImage1s[i].width, s->gImage1s[i].height, formats1 ? formats1[i] : 0u};
  c->volume_count = s->volume_count;
  return STHIP_OK;
}

extern "C" {
int sthip_create(int, sthip_ctx** out) {
  *out = g_ctx = new sthip_ctx();
  return STHIP_OK;
}
void sthip_destroy(sthip_ctx* c) {
  if (g_ctx == c) g_ctx = nullptr;
  delete c;
}
const char* sthip_last_error(const sthip_ctx* c) { return c ? c->error.c_str() : ""; }
int sthip_set_stream(sthip_ctx*, void*) { return STHIP_OK; }
int sthip_set_option(sthip_ctx*, const char*, int64_t) { return STHIP_OK; }
int sthip_scene_upload(sthip_ctx* c, const sthip_scene_desc* s) { return keep_scene(c, s, nullptr, nullptr); }
int sthip_scene_upload_formats(sthip_ctx* c, const sthip_scene_desc* s, const uint8_t* f, const uint8_t* f1) { return keep_scene(c, s, f, f1); }
int sthip_scene_update_transforms(sthip_ctx*, const sthip_TransformData*, const sthip_TransformData*, const sthip_TransformData*, uint32_t) { return STHIP_OK; }
int sthip_scene_set_material_data(sthip_ctx* c, uint32_t offset, const void* data, uint32_t bytes, sthip_images_info*) {
  c->data_calls++;
  c->data_offset = offset, c->data_bytes = bytes;
  sthip::ResidentMaterials scene;
  scene.has_scene = c->has_scene;
  scene.materials = c->materials.data();
  scene.material_bytes = c->materials.size();
  scene.instances = c->instances.data();
  scene.instance_count = (uint32_t)c->instances.size();
  scene.image_count = (uint32_t)c->images.size();
  scene.image1_count = (uint32_t)c->images1.size();
  scene.volume_count = c->volume_count;
  std::vector<uint8_t> edited;
  int code = STHIP_OK;
  if (!sthip::check_material_data(scene, offset, data, bytes, edited, code, c->error)) {
    c->refused++;
    return code;
  }
  c->materials = edited;
  return STHIP_OK;
}
int sthip_scene_set_images(sthip_ctx* c, const sthip_image_update* entries, uint32_t n, uint32_t struct_size, sthip_images_info*) {
  c->image_calls++;
  sthip::ResidentImages scene;
  scene.has_scene = c->has_scene;
  scene.images = c->images.data();
  scene.image_count = (uint32_t)c->images.size();
  scene.images1 = c->images1.data();
  scene.image1_count = (uint32_t)c->images1.size();
  int code = STHIP_OK;
  if (!sthip::check_images(scene, entries, n, struct_size, code, c->error)) {
    c->refused++;
    return code;
  }
  c->images_sent += n;
  return STHIP_OK;
}
int sthip_render(sthip_ctx*, const sthip_BDPTPushConstants*, uint32_t, uint32_t, const sthip_frame_desc*, uint32_t, uint32_t, const sthip_outputs*) { return STHIP_OK; }
int sthip_render_async(sthip_ctx*, const sthip_BDPTPushConstants*, uint32_t, uint32_t, const sthip_frame_desc*, uint32_t, uint32_t, const sthip_outputs*, uint64_t* ticket) {
  if (ticket) *ticket = 1;
  return STHIP_OK;
}
int sthip_outputs_ready(sthip_ctx*, uint64_t) { return 1; }
int sthip_wait_outputs(sthip_ctx*, uint64_t) { return STHIP_OK; }
int sthip_host_alloc(sthip_ctx*, uint64_t bytes, void** out) {
  *out = std::calloc(1, (size_t)bytes);
  return *out ? STHIP_OK : STHIP_ERR_HIP;
}
int sthip_host_free(sthip_ctx*, void* p) {
  std::free(p);
  return STHIP_OK;
}
int sthip_tonemap(sthip_ctx*, const sthip_tonemap_desc*) { return STHIP_OK; }
int sthip_write_hdr(const char*, uint32_t, uint32_t, const float*) { return STHIP_OK; }
}  // extern "C"

struct NoMaterialCalls : BDPT {  // what the multi-device driver does to its base
  explicit NoMaterialCalls(Node& node) : BDPT(node) { mMaterialsOnDevice = false; }
};

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: material_host scene.bin colour|texture|both|extent|emitter|off\n");
    return 2;
  }
  const std::string mode = argv[2];
  try {
    Reader r(argv[1]);
    NodeGraph graph;
    Node& root = graph.emplace("Instance");
    auto app = root.make_child("Application").make_component<Application>();
    LoadedScene L = load_scene(r, app.node());
    CommandBuffer cb;
    component_ptr<BDPT> renderer;
    if (mode == "off") {
      auto off = app.node().make_child("BDPT").make_component<NoMaterialCalls>();
      renderer = component_ptr<BDPT>(&off.node(), off.get());
    } else {
      renderer = app.node().make_child("BDPT").make_component<BDPT>();
    }
    app->OnRenderWindow.add_listener(renderer.node(), [&](CommandBuffer& c) { renderer->render(c, L.W, L.H, {{L.view, L.view_xf}}, 1); });
    app->run_frame(cb);  // the first frame: a full upload
    if (renderer->last_update_was_materials_only() || renderer->upload_calls() != 1) throw std::runtime_error("the first update must be an upload");
    component_ptr<Material> first, emitter;
    component_ptr<Image> image;
    L.scene_node->for_each_descendant<Material>([&](const component_ptr<Material>& m) {
      if (!first && m->emission() <= 0) first = m;
      if (!emitter && m->emission() > 0) emitter = m;
      for (int k = 0; k < 3 && !image; k++)
        if (m->values[k].image) image = m->values[k].image;
    });
    if (!first || !emitter || !image) throw std::runtime_error("the scene needs a plain material, an emitter and an image");
    if (mode == "colour" || mode == "both" || mode == "off") first->base_color()[1] = 0.125f;
    if (mode == "texture" || mode == "both") {
      if (image->is_8bit())
        for (uint8_t& b : image->bytes) b = (uint8_t)(255 - b);
      else
        for (float& v : image->pixels) v = 1.0f - v;
      image->mark_dirty();
    }
    if (mode == "extent") {
      image->width *= 2;
      (image->is_8bit() ? image->bytes.resize(image->bytes.size() * 2, 7) : image->pixels.resize(image->pixels.size() * 2, 0.5f));
      image->mark_dirty();
    }
    if (mode == "emitter") emitter->emission() = 0.0f;
    L.scene->mark_dirty();
    app->run_frame(cb);
    const sthip_ctx& c = *g_ctx;
    std::printf("MATERIALS mode=%s materials_only=%d uploads=%u data_calls=%u image_calls=%u host_data_calls=%u host_image_calls=%u data_offset=%u data_bytes=%u images_sent=%u refused=%u\n", mode.c_str(),
                renderer->last_update_was_materials_only() ? 1 : 0, c.uploads, c.data_calls, c.image_calls, renderer->material_data_calls(), renderer->image_calls(), c.data_offset, c.data_bytes, c.images_sent,
                c.refused);
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
