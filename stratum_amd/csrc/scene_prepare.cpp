// scene_prepare.cpp — see scene_prepare.h. Everything here is arithmetic over the caller's arrays; api.hip copies the results.
#include "scene_prepare.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <cmath>

namespace sthip {

bool check_scene(const sthip_scene_desc* s, const uint8_t* image_formats, const uint8_t* image1_formats, int& code, std::string& message) {
  auto bad = [&](const std::string& m) {
    code = STHIP_ERR_INVALID_ARGUMENT;
    message = m;
    return false;
  };
  auto bad_image = [](const sthip_image_desc& im) { return !im.pixels || im.width == 0 || im.height == 0 || im.width > 0xFFFF || im.height > 0xFFFF; };
  if (!s || !s->gInstances || !s->gInstanceTransforms || !s->gInstanceInverseTransforms || !s->gMaterialData || s->instance_count == 0)
    return bad("scene: a required array is NULL or there are no instances");
  if ((s->vertex_count && !s->gVertices) || (s->indices_bytes && !s->gIndices))  // a scene of sphere instances alone has neither
    return bad("scene: vertex_count / indices_bytes > 0 but the array is NULL");
  if (s->instance_count > 0xFFFF) return bad("scene: more than 65535 instances (16-bit instance index, scene.h:23)");
  if (s->light_count && !s->gLightInstances) return bad("scene: light_count > 0 but gLightInstances is NULL");
  for (uint32_t i = 0; image_formats && s->gImages && i < s->image_count; i++)
    if (image_formats[i] > STHIP_IMAGE_FORMAT_RGBA8_UNORM) return bad("scene: image_formats[" + std::to_string(i) + "] = " + std::to_string(image_formats[i]) + " is not a format of gImages");
  for (uint32_t i = 0; image1_formats && s->gImage1s && i < s->image1_count; i++)
    if (image1_formats[i] > STHIP_IMAGE_FORMAT_R8_UNORM) return bad("scene: image1_formats[" + std::to_string(i) + "] = " + std::to_string(image1_formats[i]) + " is not a format of gImage1s");
  for (uint32_t i = 0; i < s->light_count; i++)
    if (s->gLightInstances[i] >= s->instance_count) return bad("scene: gLightInstances entry out of range");
  if (s->image_count && !s->gImages) return bad("scene: image_count > 0 but gImages is NULL");
  // materials: constant values or image values over gImages (image_value.h:183-207)
  for (uint32_t i = 0; i < s->instance_count; i++) {
    const uint32_t addr = s->gInstances[i].packed[0] >> 4;
    if (instance_type(s->gInstances[i]) == STHIP_INSTANCE_TYPE_VOLUME) {  // a Medium record (Material.hpp:80-87), 40 bytes
      if ((size_t)addr + 40 > s->material_bytes || (addr & 3)) return bad("scene: medium material_address out of range");
      uint32_t vol[2];
      memcpy(vol, (const uint8_t*)s->gMaterialData + addr + 32, 8);
      if (vol[0] >= s->volume_count || (vol[1] != 0xFFFFFFFFu && vol[1] >= s->volume_count)) return bad("scene: a medium refers to a volume that is not in gVolumes");
      continue;
    }
    if ((size_t)addr + sizeof(sthip_MaterialRecord) > s->material_bytes) return bad("scene: material_address out of range");
    sthip_MaterialRecord rec;
    memcpy(&rec, (const uint8_t*)s->gMaterialData + addr, sizeof(rec));
    for (int k = 0; k < 3; k++)
      if (rec.values[k].image_index < STHIP_IMAGE_COUNT && rec.values[k].image_index >= s->image_count) return bad("scene: a material refers to an image that is not in gImages");
    if (rec.bump_index < STHIP_IMAGE_COUNT && rec.bump_index >= s->image_count) return bad("scene: a bump map refers to an image that is not in gImages");
    if (rec.alpha_mask_index < STHIP_IMAGE_COUNT && instance_type(s->gInstances[i]) == STHIP_INSTANCE_TYPE_TRIANGLES && rec.alpha_mask_index >= s->image1_count)
      return bad("scene: a material refers to an alpha mask that is not in gImage1s");
  }
  if (s->image1_count && !s->gImage1s) return bad("scene: image1_count > 0 but gImage1s is NULL");
  if (s->volume_count && !s->gVolumes) return bad("scene: volume_count > 0 but gVolumes is NULL");
  if (s->distribution_count && !s->gDistributions) return bad("scene: distribution_count > 0 but gDistributions is NULL");
  for (uint32_t i = 0; i < s->image_count; i++)
    if (bad_image(s->gImages[i])) return bad("scene: bad image");
  for (uint32_t i = 0; i < s->image1_count; i++)
    if (bad_image(s->gImage1s[i])) return bad("scene: bad alpha-mask image");
  std::vector<uint32_t> first_words;
  if (volume_first_words(*s, first_words) > 0xFFFFFFFFull) return bad("scene: gVolumes exceed 16 GiB");
  return true;
}

ImageRange scan_image_range(const void* pixels, size_t count, bool rgba8) {
  // Per-channel extremes of an image (level 0; every mip level is an average of it, and bilinear / trilinear taps are
  // convex combinations, so a sampled value lies between them): the device multiplies the constant by the texel
  // (image_value.h:194-198), so whether a material can be specular depends on the texels.
  ImageRange r;
  const float* px = rgba8 ? nullptr : static_cast<const float*>(pixels);
  const uint8_t* px8 = rgba8 ? static_cast<const uint8_t*>(pixels) : nullptr;  // RGBA8: the decoded bytes
  for (int c = 0; c < 4; c++) {
    float a = __builtin_inff(), b = -__builtin_inff();
    bool nan = false;
    for (size_t k = 0; pixels && k < count; k++) {
      const float t = px8 ? (float)px8[4 * k + c] / 255.0f : px[4 * k + c];
      if (t != t) nan = true;
      a = std::min(a, t);
      b = std::max(b, t);
    }
    if (nan) r.nan_mask |= 1u << c;
    if (nan || !pixels || !count) a = -__builtin_inff(), b = __builtin_inff();  // unknown: everything is possible
    r.lo[c] = a;
    r.hi[c] = b;
  }
  r.known = 1;
  return r;
}

// the images whose range value_range below reads: metallic and roughness (values[1]), transmission (values[2])
static bool reads_range(const sthip_MaterialRecord& rec, int k, uint32_t image_count) {
  const uint32_t index = rec.values[k].image_index;
  if (index >= STHIP_IMAGE_COUNT || index >= image_count) return false;
  const float* v = rec.values[k].value;
  return v[0] > 0 || v[1] > 0 || v[2] > 0 || v[3] > 0;
}

void material_images(const MaterialInstance* instances, uint32_t instance_count, const uint8_t* materials, uint32_t image_count, std::vector<uint8_t>& named, std::vector<uint8_t>& range_read) {
  named.assign(image_count, 0);
  range_read.assign(image_count, 0);
  for (uint32_t i = 0; i < instance_count; i++) {
    if (instances[i].type == STHIP_INSTANCE_TYPE_VOLUME) continue;
    sthip_MaterialRecord rec;
    memcpy(&rec, materials + instances[i].address, sizeof(rec));
    for (int k = 0; k < 4; k++) {
      const uint32_t index = k < 3 ? rec.values[k].image_index : rec.bump_index;
      if (index < image_count) named[index] = 1;
    }
    for (int k = 1; k < 3; k++)
      if (reads_range(rec, k, image_count)) range_read[rec.values[k].image_index] = 1;
  }
}

MaterialAnalysis analyse_materials(const sthip_scene_desc& s, const uint8_t* image_formats) {
  std::vector<MaterialInstance> instances(s.instance_count);
  for (uint32_t i = 0; i < s.instance_count; i++) instances[i] = MaterialInstance{s.gInstances[i].packed[0] >> 4, instance_type(s.gInstances[i])};
  std::vector<uint8_t> named, range_read;
  material_images(instances.data(), s.instance_count, (const uint8_t*)s.gMaterialData, s.image_count, named, range_read);
  std::vector<ImageRange> ranges(s.image_count);
  for (uint32_t i = 0; i < s.image_count; i++)
    if (range_read[i]) ranges[i] = scan_image_range(s.gImages[i].pixels, (size_t)s.gImages[i].width * s.gImages[i].height, image_formats && image_formats[i]);
  MaterialAnalysis m = analyse_materials(instances.data(), s.instance_count, (const uint8_t*)s.gMaterialData, s.image_count, ranges.data());
  m.image_ranges = std::move(ranges);
  return m;
}

MaterialAnalysis analyse_materials(const MaterialInstance* instances, uint32_t instance_count, const uint8_t* materials, uint32_t image_count, const ImageRange* ranges) {
  MaterialAnalysis m;
  auto image_range = [&](uint32_t index, int channel, float& lo, float& hi) {
    lo = -__builtin_inff(), hi = __builtin_inff();  // an image nobody scanned: everything is possible
    if (ranges[index].known) lo = ranges[index].lo[channel], hi = ranges[index].hi[channel];
  };
  // bounds of one component of an image value: constant, or constant * texel (zero when no component of the constant is positive)
  auto value_range = [&](const sthip_MaterialRecord& rec, int k, int channel, float& lo, float& hi) {
    const float c = rec.values[k].value[channel];
    lo = hi = c;
    const uint32_t index = rec.values[k].image_index;
    if (index >= STHIP_IMAGE_COUNT || index >= image_count) return;
    const float* v = rec.values[k].value;
    if (!(v[0] > 0 || v[1] > 0 || v[2] > 0 || v[3] > 0)) {
      lo = hi = 0.0f;
      return;
    }
    float a, b;
    image_range(index, channel, a, b);
    lo = std::min(c * a, c * b);
    hi = std::max(c * a, c * b);
    if (lo != lo || hi != hi) lo = -__builtin_inff(), hi = __builtin_inff();
  };
  m.inst_flags.assign(std::max<uint32_t>(1, instance_count), (uint8_t)INST_FLAG_KEEP);  // k_cull_terminal's table (kernels.h)
  m.instance_is_volume.assign(instance_count, 0);
  m.image_in_material.assign(image_count, 0);
  for (uint32_t i = 0; i < instance_count; i++) {
    const uint32_t addr = instances[i].address, type = instances[i].type;
    if (type == STHIP_INSTANCE_TYPE_SPHERE) m.has_spheres = true;
    if (type == STHIP_INSTANCE_TYPE_VOLUME) {  // a Medium record (Material.hpp:80-87), 40 bytes
      m.has_volumes = true;
      m.volume_instances++;
      m.instance_is_volume[i] = 1;
      float anisotropy;
      memcpy(&anisotropy, materials + addr + 12, 4);
      if (!(fabsf(anisotropy) <= 0.999f)) m.has_specular = true;  // Medium::is_specular (medium.hlsli:22): its vertices are not diffuse vertices
      continue;
    }
    sthip_MaterialRecord rec;
    memcpy(&rec, materials + addr, sizeof(rec));
    for (int k = 0; k < 3; k++)
      if (rec.values[k].image_index < STHIP_IMAGE_COUNT) m.textured = true;
    if (rec.bump_index < STHIP_IMAGE_COUNT) m.textured = true;
    for (int k = 0; k < 4; k++) {
      const uint32_t index = k < 3 ? rec.values[k].image_index : rec.bump_index;
      if (index < image_count) m.image_in_material[index] = 1;
    }
    if (rec.alpha_mask_index < STHIP_IMAGE_COUNT && type == STHIP_INSTANCE_TYPE_TRIANGLES) m.any_alpha = true;
    // DisneyMaterial::is_specular (disney_material.hlsli:125) is evaluated per hit on value * texel, so the host test is
    // over what the product can reach: conservative (a "maybe" only costs bounce rounds that find empty queues)
    float lo, metallic_hi, roughness_lo, transmission_hi;
    value_range(rec, 1, 0, lo, metallic_hi);
    value_range(rec, 1, 1, roughness_lo, lo);
    value_range(rec, 2, 2, lo, transmission_hi);
    if ((metallic_hi > 0.999f || transmission_hi > 0.999f) && roughness_lo <= 1e-2f) m.has_specular = true;
    if (type == STHIP_INSTANCE_TYPE_TRIANGLES || type == STHIP_INSTANCE_TYPE_SPHERE) {
      // what DisneyMaterial::load reads of an untextured record (shading.h), with the device's arithmetic: Le = base_color *
      // emission, can_eval, is_specular (only the untextured k_shade instantiations, i.e. a scene without images, consult this)
      float f[14];
      memcpy(f, materials + addr, sizeof(f));
      const float le[3] = {f[0] * f[3], f[1] * f[3], f[2] * f[3]};
      const bool emits = le[0] > 0 || le[1] > 0 || le[2] > 0;
      const bool can_eval = f[3] <= 0 && (f[0] > 0 || f[1] > 0 || f[2] > 0);
      const bool specular = (f[5] > 0.999f || f[12] > 0.999f) && f[6] <= 1e-2f;
      m.inst_flags[i] = (uint8_t)((emits ? INST_FLAG_EMITS : 0) | (can_eval ? INST_FLAG_CAN_EVAL : 0) | (specular ? INST_FLAG_SPECULAR : 0));
    }
  }
  return m;
}

bool check_environment(const ResidentEnvironmentScene& scene, const sthip_environment_desc* d, EnvironmentPlan& plan, int& code, std::string& message) {
  auto refuse = [&](int c, const std::string& m) {
    code = c;
    message = "sthip_scene_set_environment: " + m;
    return false;
  };
  auto bad = [&](const std::string& m) { return refuse(STHIP_ERR_INVALID_ARGUMENT, m); };
  plan = EnvironmentPlan();
  if (!d) return bad("the description is NULL");
  if (d->struct_size != sizeof(sthip_environment_desc)) return bad("struct_size is " + std::to_string(d->struct_size) + ", not sizeof(sthip_environment_desc) = " + std::to_string(sizeof(sthip_environment_desc)));
  if (!scene.has_scene || !scene.materials) return bad("no scene is resident (before sthip_scene_upload)");
  const size_t addr = d->material_address;
  if ((addr & 3) || addr + 16 > scene.material_bytes) return bad("material_address is unaligned or outside gMaterialData");
  uint32_t rec[8] = {0};
  memcpy(rec, scene.materials + addr, 16);
  plan.has_image = rec[3] < STHIP_IMAGE_COUNT;
  plan.set_value = d->value != nullptr;
  plan.replace_pixels = d->pixels != nullptr;
  plan.build_tables = plan.replace_pixels || !plan.set_value;
  if (plan.set_value && d->value[0] == 0 && d->value[1] == 0 && d->value[2] == 0) return bad("value is zero: upstream stores no record for a zero environment (upload the scene without one)");
  if (!plan.has_image) {
    if (plan.replace_pixels) return bad("pixels for an environment record without an image");
    plan.build_tables = false;  // (a constant environment has no tables: nothing to build)
    return true;
  }
  if (rec[3] >= scene.image_count || addr + 32 > scene.material_bytes) return bad("the record refers to an image that is not in gImages, or its table offsets lie outside gMaterialData");
  memcpy(rec, scene.materials + addr, 32);
  const DeviceImage& im = scene.images[rec[3]];
  plan.image_index = rec[3];
  plan.width = im.w[0];
  plan.height = im.h[0];
  if (plan.replace_pixels && (d->width != plan.width || d->height != plan.height))
    return bad("the extent " + std::to_string(d->width) + " x " + std::to_string(d->height) + " differs from the resident image's " + std::to_string(plan.width) + " x " + std::to_string(plan.height) +
               " (a change of extent is an upload)");
  const size_t w = plan.width, h = plan.height;
  const size_t need[4] = {h, w * h, h + 1, (w + 1) * h};  // marginal_pdf, row_pdf, marginal_cdf, row_cdf (dist2.h)
  for (int k = 0; k < 4; k++) {
    plan.table[k] = rec[4 + k];
    if ((size_t)rec[4 + k] + need[k] > scene.distribution_count) return bad("an environment distribution table lies outside gDistributions");
  }
  for (int k = 0; k < 4; k++)
    for (int j = k + 1; j < 4; j++)
      if ((size_t)rec[4 + k] < (size_t)rec[4 + j] + need[j] && (size_t)rec[4 + j] < (size_t)rec[4 + k] + need[k]) return bad("two distribution tables of the record overlap");
  if (im.format != STHIP_IMAGE_FORMAT_RGBA32F)
    return refuse(STHIP_ERR_UNSUPPORTED, "the environment map is an 8-bit image (gImages[" + std::to_string(rec[3]) + "] is RGBA8_UNORM): upload it as RGBA32F");
  if (plan.replace_pixels && scene.image_in_material && scene.image_in_material[rec[3]])
    return refuse(STHIP_ERR_UNSUPPORTED, "gImages[" + std::to_string(rec[3]) + "] is also named by a material record: its texels decided the kernels of the scene (upload the scene again)");
  return true;
}

bool check_images(const ResidentImages& scene, const sthip_image_update* entries, uint32_t n, uint32_t struct_size, int& code, std::string& message) {
  auto bad = [&](const std::string& m) {
    code = STHIP_ERR_INVALID_ARGUMENT;
    message = "sthip_scene_set_images: " + m;
    return false;
  };
  if (struct_size != sizeof(sthip_image_update)) return bad("struct_size is " + std::to_string(struct_size) + ", not sizeof(sthip_image_update) = " + std::to_string(sizeof(sthip_image_update)));
  if (!scene.has_scene) return bad("no scene is resident (before sthip_scene_upload)");
  if (n && !entries) return bad("entries is NULL");
  for (uint32_t k = 0; k < n; k++) {
    const sthip_image_update& e = entries[k];
    const std::string at = "entries[" + std::to_string(k) + "]: ";
    if (e.which > 1) return bad(at + "which is " + std::to_string(e.which) + " (0 = gImages, 1 = gImage1s)");
    const uint32_t count = e.which ? scene.image1_count : scene.image_count;
    const char* array = e.which ? "gImage1s" : "gImages";
    if (e.index >= count) return bad(at + "index " + std::to_string(e.index) + " is not in " + array);
    if (!e.pixels) return bad(at + "pixels is NULL");
    const uint32_t w = e.which ? scene.images1[e.index].w : scene.images[e.index].w[0], h = e.which ? scene.images1[e.index].h : scene.images[e.index].h[0];
    if (e.width != w || e.height != h)
      return bad(at + "the extent " + std::to_string(e.width) + " x " + std::to_string(e.height) + " differs from the resident image's " + std::to_string(w) + " x " + std::to_string(h) + " (a change of extent is an upload)");
    for (uint32_t j = 0; j < k; j++)
      if (entries[j].which == e.which && entries[j].index == e.index) return bad(at + array + "[" + std::to_string(e.index) + "] is named twice in one call");
    const bool rgba32f = !e.which && scene.images[e.index].format == STHIP_IMAGE_FORMAT_RGBA32F;
    if (e.device_ptr && ((uintptr_t)e.pixels & (rgba32f ? 15u : 3u))) return bad(at + "the device pointer is not aligned to " + (rgba32f ? "16" : "4") + " bytes");
  }
  return true;
}

bool check_material_data(const ResidentMaterials& scene, uint32_t offset, const void* data, uint32_t bytes, std::vector<uint8_t>& edited, int& code, std::string& message) {
  auto refuse = [&](int c, const std::string& m) {
    code = c;
    message = "sthip_scene_set_material_data: " + m;
    return false;
  };
  auto bad = [&](const std::string& m) { return refuse(STHIP_ERR_INVALID_ARGUMENT, m); };
  auto unsupported = [&](uint32_t i, const std::string& m) { return refuse(STHIP_ERR_UNSUPPORTED, "instance " + std::to_string(i) + ": " + m + " (upload the scene again)"); };
  if (!scene.has_scene || !scene.materials) return bad("no scene is resident (before sthip_scene_upload)");
  if (bytes && !data) return bad("data is NULL");
  if ((offset & 3) || (bytes & 3)) return bad("offset and bytes must be multiples of 4");
  if ((size_t)offset + bytes > scene.material_bytes) return bad("the range [" + std::to_string(offset) + ", " + std::to_string((size_t)offset + bytes) + ") ends past the " + std::to_string(scene.material_bytes) + " bytes of gMaterialData");
  edited.assign(scene.materials, scene.materials + scene.material_bytes);
  if (bytes) memcpy(edited.data() + offset, data, bytes);
  auto emits = [](const uint8_t* record) {  // (analyse_materials: Le = base_color * emission of the untextured record)
    float f[4];
    memcpy(f, record, sizeof(f));
    return f[0] * f[3] > 0 || f[1] * f[3] > 0 || f[2] * f[3] > 0;
  };
  for (uint32_t i = 0; i < scene.instance_count; i++) {
    const uint32_t addr = scene.instances[i].address, type = scene.instances[i].type;
    const size_t size = type == STHIP_INSTANCE_TYPE_VOLUME ? 40 : sizeof(sthip_MaterialRecord);
    if ((size_t)addr + size <= offset || (size_t)offset + bytes <= addr) continue;  // (the record lies outside the edit)
    if (type == STHIP_INSTANCE_TYPE_VOLUME) {
      uint32_t vol[2], old[2];
      memcpy(vol, edited.data() + addr + 32, 8);
      memcpy(old, scene.materials + addr + 32, 8);
      if (vol[0] >= scene.volume_count || (vol[1] != 0xFFFFFFFFu && vol[1] >= scene.volume_count)) return bad("a medium refers to a volume that is not in gVolumes");
      if (vol[0] != old[0] || vol[1] != old[1]) return unsupported(i, "the volume indices of a medium change");
      continue;
    }
    sthip_MaterialRecord rec, was;
    memcpy(&rec, edited.data() + addr, sizeof(rec));
    memcpy(&was, scene.materials + addr, sizeof(was));
    for (int k = 0; k < 3; k++)
      if (rec.values[k].image_index < STHIP_IMAGE_COUNT && rec.values[k].image_index >= scene.image_count) return bad("a material refers to an image that is not in gImages");
    if (rec.bump_index < STHIP_IMAGE_COUNT && rec.bump_index >= scene.image_count) return bad("a bump map refers to an image that is not in gImages");
    if (type == STHIP_INSTANCE_TYPE_TRIANGLES) {
      if (rec.alpha_mask_index < STHIP_IMAGE_COUNT && rec.alpha_mask_index >= scene.image1_count) return bad("a material refers to an alpha mask that is not in gImage1s");
      if (rec.alpha_mask_index != was.alpha_mask_index) return unsupported(i, "the alpha_mask_index of a triangle instance changes (the mask is in the tree)");
    }
    if ((type == STHIP_INSTANCE_TYPE_TRIANGLES || type == STHIP_INSTANCE_TYPE_SPHERE) && emits(edited.data() + addr) != emits(scene.materials + addr))
      return unsupported(i, "its emission appears or disappears (the light list and the emitter bounds are the upload's)");
  }
  return true;
}

void environment_row_sines(uint32_t height, std::vector<double>& out) {
  out.resize(height);
  const float inv_height = 1 / (float)height;
  for (uint32_t y = 0; y < height; y++) out[y] = std::sin(M_PI * (y + 0.5f) * inv_height);
}

bool check_vertex_streams(bool has_scene, uint32_t scene_vertex_count, const sthip_vertex_streams* d, int& code, std::string& message) {
  auto bad = [&](const std::string& m) {
    code = STHIP_ERR_INVALID_ARGUMENT;
    message = "sthip_scene_set_vertices: " + m;
    return false;
  };
  if (!has_scene) return bad("no scene is resident (before sthip_scene_upload)");
  if (!d) return bad("the description is NULL");
  if (d->struct_size < sizeof(sthip_vertex_streams)) return bad("struct_size is " + std::to_string(d->struct_size) + ", below sizeof(sthip_vertex_streams) = " + std::to_string(sizeof(sthip_vertex_streams)));
  if (!d->positions) return bad("positions is NULL");
  if ((uint64_t)d->first_vertex + d->vertex_count > scene_vertex_count) return bad("first_vertex + vertex_count ends past the vertex_count of the uploaded scene");
  struct Stream {
    const char* name;
    const void* p;
    uint32_t stride, element;
  };
  const Stream streams[3] = {{"position", d->positions, d->position_stride, 12}, {"normal", d->normals, d->normal_stride, 12}, {"texcoord", d->texcoords, d->texcoord_stride, 8}};
  for (const Stream& s : streams) {
    if (!s.p) continue;  // (the stride of an absent stream is not read)
    const std::string field = std::string(s.name) + "s", stride = std::string(s.name) + "_stride";
    if ((uintptr_t)s.p & 3) return bad(field + " is not 4-byte aligned");
    if (s.stride & 3) return bad(stride + " = " + std::to_string(s.stride) + " is not a multiple of 4");
    if (s.stride < s.element) return bad(stride + " = " + std::to_string(s.stride) + " is below the element size " + std::to_string(s.element));
  }
  if (d->normals && d->recompute_normals) return bad("normals together with recompute_normals");
  return true;
}

std::vector<VertexMesh> list_vertex_meshes(const sthip_InstanceData* instances, uint32_t instance_count) {
  std::vector<VertexMesh> out;
  for (uint32_t i = 0; instances && i < instance_count; i++) {
    const sthip_InstanceData& in = instances[i];
    if (instance_type(in) != STHIP_INSTANCE_TYPE_TRIANGLES) continue;
    out.push_back(VertexMesh{in.packed[3], in.packed[2], in.packed[1] >> 28, (in.packed[1] >> 12) & 0xFFFFu});
  }
  auto key = [](const VertexMesh& m) { return std::array<uint32_t, 4>{{m.indices_byte_offset, m.first_vertex, m.index_stride, m.prim_count}}; };
  std::sort(out.begin(), out.end(), [&](const VertexMesh& a, const VertexMesh& b) { return key(a) < key(b); });
  out.erase(std::unique(out.begin(), out.end(), [&](const VertexMesh& a, const VertexMesh& b) { return key(a) == key(b); }), out.end());
  return out;
}

bool pad_emitter_bounds(EmitterBounds& b) {
  double diag = 0;
  for (int a = 0; a < 3; a++) {
    const float mag = std::max(fabsf(b.lo[a]), fabsf(b.hi[a])) * (1.0f / 32768.0f) + 1e-30f;
    b.lo[a] -= mag;
    b.hi[a] += mag;
    b.sphere[a] = 0.5f * b.lo[a] + 0.5f * b.hi[a];
    diag += ((double)b.hi[a] - b.lo[a]) * ((double)b.hi[a] - b.lo[a]);
  }
  b.sphere[3] = (float)sqrt(diag);  // (twice the box's own radius: the padding only has to be large enough)
  return std::isfinite(b.sphere[3]);
}

void emitter_bounds(const sthip_scene_desc& s, const std::vector<uint8_t>& inst_flags, std::vector<EmitterBounds>& out) {
  out.clear();
  bool usable = true;
  for (uint32_t i = 0; i < s.instance_count && usable; i++) {
    // (sphere lights, environments: scenes of the extended k_shade instantiation, which does not answer last rays)
    if (instance_type(s.gInstances[i]) != STHIP_INSTANCE_TYPE_TRIANGLES || !(inst_flags[i] & INST_FLAG_EMITS)) continue;
    if (out.size() == STHIP_MAX_EMITTER_BOUNDS) {
      usable = false;
      break;
    }
    const uint32_t prims = (s.gInstances[i].packed[1] >> 12) & 0xFFFFu, stride = s.gInstances[i].packed[1] >> 28;
    const uint32_t first_vertex = s.gInstances[i].packed[2];
    const uint8_t* ib = (const uint8_t*)s.gIndices + s.gInstances[i].packed[3];
    EmitterBounds b{};
    for (int a = 0; a < 3; a++) b.lo[a] = __builtin_inff(), b.hi[a] = -__builtin_inff();
    for (uint32_t k = 0; k < 3 * prims; k++) {
      uint32_t index;
      if (stride == 2) {
        uint16_t w;
        memcpy(&w, ib + 2 * (size_t)k, 2);
        index = w;
      } else {
        memcpy(&index, ib + 4 * (size_t)k, 4);
      }
      if ((size_t)first_vertex + index >= s.vertex_count) {  // (the builders have refused such a scene already)
        usable = false;
        break;
      }
      const float* pos = s.gVertices[first_vertex + index].position;
      for (int a = 0; a < 3; a++) {
        b.lo[a] = std::min(b.lo[a], pos[a]);
        b.hi[a] = std::max(b.hi[a], pos[a]);
      }
    }
    if (!prims || !(b.lo[0] <= b.hi[0])) continue;  // (no triangle: nothing to hit)
    if (!pad_emitter_bounds(b)) usable = false;
    b.instance = i;
    static const float ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    b.identity = (!memcmp(&s.gInstanceTransforms[i], ident, 48) && !memcmp(&s.gInstanceInverseTransforms[i], ident, 48)) ? 1u : 0u;
    out.push_back(b);
  }
  if (!usable) out.clear();
}

// images: mip chain by 2x2 box filter, level k+1 = max(1, floor(dim / 2)), ((a + b) + (c + d)) * 0.25
// (RGBA8 images, sthip_scene_upload_formats: the same shape in an array of their own, (a + b + c + d + 2) >> 2 per channel,
// made on the device from level 0 — mips.hip)
ImageLayout layout_images(const sthip_scene_desc& s, const uint8_t* image_formats) {
  ImageLayout out;
  std::vector<DeviceImage>& table = out.table;
  std::vector<float>& texels = out.texels;
  size_t& texels8 = out.texels8;  // words of image_texels8
  table.resize(s.image_count);
  for (uint32_t i = 0; i < s.image_count; i++) {
    uint32_t w = s.gImages[i].width, h = s.gImages[i].height;
    DeviceImage& im = table[i];
    memset(&im, 0, sizeof(im));
    if (image_formats && image_formats[i] == STHIP_IMAGE_FORMAT_RGBA8_UNORM) {  // the layout only: the texels go up from the caller's array
      im.format = STHIP_IMAGE_FORMAT_RGBA8_UNORM;
      for (uint32_t level = 0;; level++) {
        im.offset[level] = (uint32_t)texels8;
        im.w[level] = (uint16_t)w;
        im.h[level] = (uint16_t)h;
        im.levels = level + 1;
        texels8 += (size_t)w * h;
        if ((w == 1 && h == 1) || level + 1 == STHIP_MAX_MIPS) break;
        w = std::max(1u, w / 2);
        h = std::max(1u, h / 2);
      }
      if (texels8 > 0xFFFFFFFFull) {
        out.error = "scene: the RGBA8 images exceed 2^32 texels (32-bit texel offsets)";
        return out;
      }
      continue;
    }
    size_t level_start = texels.size();
    texels.insert(texels.end(), s.gImages[i].pixels, s.gImages[i].pixels + (size_t)w * h * 4);
    for (uint32_t level = 0;; level++) {
      im.offset[level] = (uint32_t)(level_start / 4);
      im.w[level] = (uint16_t)w;
      im.h[level] = (uint16_t)h;
      im.levels = level + 1;
      if ((w == 1 && h == 1) || level + 1 == STHIP_MAX_MIPS) break;
      const uint32_t nw = std::max(1u, w / 2), nh = std::max(1u, h / 2);
      const size_t next_start = texels.size();
      texels.resize(next_start + (size_t)nw * nh * 4);
      const float* prev = texels.data() + level_start;
      float* next = texels.data() + next_start;
      for (uint32_t y = 0; y < nh; y++)
        for (uint32_t x = 0; x < nw; x++) {
          const uint32_t x0 = std::min(2 * x, w - 1), x1 = std::min(2 * x + 1, w - 1), y0 = std::min(2 * y, h - 1), y1 = std::min(2 * y + 1, h - 1);
          for (int k = 0; k < 4; k++) {
            const float a = prev[4 * ((size_t)y0 * w + x0) + k], b = prev[4 * ((size_t)y0 * w + x1) + k];
            const float c = prev[4 * ((size_t)y1 * w + x0) + k], e = prev[4 * ((size_t)y1 * w + x1) + k];
            next[4 * ((size_t)y * nw + x) + k] = ((a + b) + (c + e)) * 0.25f;
          }
        }
      level_start = next_start;
      w = nw;
      h = nh;
    }
  }
  return out;
}

MaskLayout layout_alpha_masks(const sthip_scene_desc& s, const uint8_t* image1_formats) {
  MaskLayout out;
  out.table.resize(s.image1_count);
  for (uint32_t i = 0; i < s.image1_count; i++) {
    const sthip_image_desc& im = s.gImage1s[i];
    out.table[i].w = im.width;
    out.table[i].h = im.height;
    if (image1_formats && image1_formats[i] == STHIP_IMAGE_FORMAT_R8_UNORM) {
      const uint8_t* bytes = reinterpret_cast<const uint8_t*>(im.pixels);
      out.table[i].offset = (uint32_t)out.texels8.size();
      out.table[i].format = STHIP_IMAGE_FORMAT_R8_UNORM;
      out.texels8.insert(out.texels8.end(), bytes, bytes + (size_t)im.width * im.height);
      if (out.texels8.size() > 0xFFFFFFFFull) {
        out.error = "scene: the R8 alpha masks exceed 2^32 texels (32-bit texel offsets)";
        return out;
      }
      continue;
    }
    out.table[i].offset = (uint32_t)out.texels.size();
    out.table[i].format = STHIP_IMAGE_FORMAT_R32F;
    out.texels.insert(out.texels.end(), im.pixels, im.pixels + (size_t)im.width * im.height);
  }
  return out;
}

size_t volume_first_words(const sthip_scene_desc& s, std::vector<uint32_t>& out) {
  out.resize(s.volume_count);
  size_t words = 0;
  for (uint32_t i = 0; i < s.volume_count; i++) {
    out[i] = (uint32_t)words;
    words += (size_t)(s.gVolumes[i].bytes / 4);
  }
  return words;
}

}  // namespace sthip
