// material_update_check.cpp — the host part of sthip_scene_set_images / sthip_scene_set_material_data
// (stratum_amd/csrc/scene_prepare.cpp: check_images, check_material_data, scan_image_range, material_images and the analysis
// with supplied ranges) as a plain CPU program with its own main, so that it runs under -fsanitize=address,undefined. It links
// scene_prepare.cpp only. Every case prints "ok <name>" or "FAIL <name>"; the last line is "MATERIAL UPDATE CHECK OK" when all
// passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../stratum_amd/csrc/scene_prepare.h"

static int failures = 0;
static void report(const char* name, bool pass, const std::string& detail = "", bool always = false) {
  const bool show = !detail.empty() && (always || !pass);  // (an accepted call leaves the message of the refusal before it)
  std::printf("%s %s%s%s\n", pass ? "ok  " : "FAIL", name, show ? ": " : "", show ? detail.c_str() : "");
  if (!pass) failures++;
}

// A scene of `n` triangle instances, one record each, with `images` RGBA images of 4 x 3 texels
struct Scene {
  std::vector<sthip_InstanceData> instances;
  std::vector<uint8_t> materials;
  std::vector<std::vector<float>> floats;
  std::vector<std::vector<uint8_t>> bytes;
  std::vector<sthip_image_desc> images;
  std::vector<uint8_t> formats;
  sthip_scene_desc d{};

  uint32_t add_record(uint32_t type, const sthip_MaterialRecord& rec) {
    const uint32_t addr = (uint32_t)materials.size();
    materials.resize(addr + sizeof(rec));
    memcpy(materials.data() + addr, &rec, sizeof(rec));
    sthip_InstanceData inst{};
    inst.packed[0] = type | (addr << 4);
    instances.push_back(inst);
    return addr;
  }
  uint32_t add_medium(float anisotropy, uint32_t vol0, uint32_t vol1) {
    const uint32_t addr = (uint32_t)materials.size();
    materials.resize(addr + 40, 0);
    memcpy(materials.data() + addr + 12, &anisotropy, 4);
    memcpy(materials.data() + addr + 32, &vol0, 4);
    memcpy(materials.data() + addr + 36, &vol1, 4);
    sthip_InstanceData inst{};
    inst.packed[0] = STHIP_INSTANCE_TYPE_VOLUME | (addr << 4);
    instances.push_back(inst);
    return addr;
  }
  void add_float_image(const std::vector<float>& px) {
    floats.push_back(px);
    bytes.emplace_back();
    formats.push_back(STHIP_IMAGE_FORMAT_RGBA32F);
  }
  void add_byte_image(const std::vector<uint8_t>& px) {
    floats.emplace_back();
    bytes.push_back(px);
    formats.push_back(STHIP_IMAGE_FORMAT_RGBA8_UNORM);
  }
  const sthip_scene_desc& desc() {
    images.clear();
    for (size_t i = 0; i < formats.size(); i++)
      images.push_back(sthip_image_desc{formats[i] ? reinterpret_cast<const float*>(bytes[i].data()) : floats[i].data(), 4, 3});
    d = sthip_scene_desc{};
    d.gInstances = instances.data();
    d.instance_count = (uint32_t)instances.size();
    d.gMaterialData = materials.data();
    d.material_bytes = (uint32_t)materials.size();
    d.gImages = images.data();
    d.image_count = (uint32_t)images.size();
    return d;
  }
};

static sthip_MaterialRecord record(float metallic, float roughness, uint32_t image1 = 0xFFFFFFFFu) {
  sthip_MaterialRecord r{};
  const float base[4] = {0.5f, 0.5f, 0.5f, 0.0f}, data1[4] = {metallic, roughness, 0, 0}, data2[4] = {0, 1, 0, 1.5f};
  memcpy(r.values[0].value, base, 16);
  memcpy(r.values[1].value, data1, 16);
  memcpy(r.values[2].value, data2, 16);
  r.values[0].image_index = r.values[2].image_index = 0xFFFFFFFFu;
  r.values[1].image_index = image1;
  r.alpha_mask_index = r.bump_index = 0xFFFFFFFFu;
  return r;
}

static std::vector<float> float_image(float metallic, float roughness) {
  std::vector<float> px(4 * 3 * 4);
  for (size_t k = 0; k < 12; k++) px[4 * k] = metallic, px[4 * k + 1] = roughness, px[4 * k + 2] = 0.25f, px[4 * k + 3] = 1.0f;
  return px;
}

static bool same_analysis(const sthip::MaterialAnalysis& a, const sthip::MaterialAnalysis& b) {
  return a.has_specular == b.has_specular && a.textured == b.textured && a.any_alpha == b.any_alpha && a.has_spheres == b.has_spheres && a.has_volumes == b.has_volumes &&
         a.volume_instances == b.volume_instances && a.instance_is_volume == b.instance_is_volume && a.inst_flags == b.inst_flags && a.image_in_material == b.image_in_material;
}

// analyse_materials(scene) against the analysis with ranges supplied for every image a record names (what the context does after
// a device scan), and the verdict the case is made for
static void analysis_case(const char* name, Scene& sc, bool want_specular) {
  const sthip_scene_desc& d = sc.desc();
  const sthip::MaterialAnalysis whole = sthip::analyse_materials(d, sc.formats.data());
  std::vector<sthip::MaterialInstance> inst(d.instance_count);
  for (uint32_t i = 0; i < d.instance_count; i++) inst[i] = sthip::MaterialInstance{d.gInstances[i].packed[0] >> 4, d.gInstances[i].packed[0] & 0xFu};
  std::vector<uint8_t> named, range_read;
  sthip::material_images(inst.data(), d.instance_count, sc.materials.data(), d.image_count, named, range_read);
  std::vector<sthip::ImageRange> ranges(d.image_count);
  for (uint32_t i = 0; i < d.image_count; i++)
    if (named[i]) ranges[i] = sthip::scan_image_range(d.gImages[i].pixels, 12, sc.formats[i] != 0);
  const sthip::MaterialAnalysis split = sthip::analyse_materials(inst.data(), d.instance_count, sc.materials.data(), d.image_count, ranges.data());
  bool pass = same_analysis(whole, split) && whole.has_specular == want_specular && named == whole.image_in_material;
  for (uint32_t i = 0; i < d.image_count; i++) {  // the upload keeps the ranges it scanned: those the analysis reads
    pass = pass && whole.image_ranges.size() == d.image_count && (whole.image_ranges[i].known != 0) == (range_read[i] != 0);
    if (pass && range_read[i]) pass = !memcmp(whole.image_ranges[i].lo, ranges[i].lo, 16) && !memcmp(whole.image_ranges[i].hi, ranges[i].hi, 16) && whole.image_ranges[i].nan_mask == ranges[i].nan_mask;
  }
  report(name, pass);
}

static void analysis_cases() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  {  // float images: a rough metal and a mirror
    Scene sc;
    sc.add_float_image(float_image(1.0f, 0.5f));
    sc.add_record(STHIP_INSTANCE_TYPE_TRIANGLES, record(1, 1, 0));
    analysis_case("float image, rough", sc, false);
    sc.floats[0][4 * 7 + 1] = 0.005f;  // one smooth texel
    analysis_case("float image, mirror", sc, true);
  }
  {  // 8-bit images
    Scene sc;
    std::vector<uint8_t> px(48, 255);
    for (size_t k = 0; k < 12; k++) px[4 * k + 1] = 128;
    sc.add_byte_image(px);
    sc.add_record(STHIP_INSTANCE_TYPE_TRIANGLES, record(1, 1, 0));
    analysis_case("8-bit image, rough", sc, false);
    sc.bytes[0][4 * 11 + 1] = 2;  // 2 / 255 <= 1e-2
    analysis_case("8-bit image, mirror", sc, true);
    sc.bytes[0][4 * 11 + 1] = 3;  // 3 / 255 > 1e-2
    analysis_case("8-bit image, just rough", sc, false);
  }
  {  // a NaN makes its channel unknown: the roughness could be anything, the metallic channel decides
    Scene sc;
    sc.add_float_image(float_image(1.0f, 0.5f));
    sc.floats[0][4 * 5 + 1] = nan;
    sc.add_record(STHIP_INSTANCE_TYPE_TRIANGLES, record(1, 1, 0));
    analysis_case("image with a NaN", sc, true);
    const sthip::ImageRange r = sthip::scan_image_range(sc.floats[0].data(), 12, false);
    report("NaN channel is -inf / +inf, the others are exact", r.nan_mask == 2u && r.lo[1] == -inf && r.hi[1] == inf && r.lo[0] == 1.0f && r.hi[0] == 1.0f && r.lo[2] == 0.25f && r.known == 1);
    sc.floats[0] = float_image(0.5f, 0.5f);
    sc.floats[0][4 * 5 + 1] = nan;
    analysis_case("image with a NaN, not metallic", sc, false);
  }
  {  // no positive component in the constant: the value is zero whatever the texels say, and nobody scans the image
    Scene sc;
    sc.add_float_image(float_image(1.0f, 0.0f));
    sthip_MaterialRecord rec = record(0, 0, 0);
    rec.values[1].value[0] = -1.0f;
    sc.add_record(STHIP_INSTANCE_TYPE_TRIANGLES, rec);
    analysis_case("constant without a positive component", sc, false);
    const sthip::MaterialAnalysis m = sthip::analyse_materials(sc.desc(), sc.formats.data());
    report("... its image is named but not scanned", m.image_in_material[0] == 1 && m.image_ranges[0].known == 0 && m.textured);
  }
  {  // infinities and denormals are kept; an untextured specular record, a sphere and a medium ride along
    Scene sc;
    std::vector<float> px = float_image(0.5f, 0.5f);
    px[0] = inf, px[4 * 3 + 1] = -inf, px[4 * 9 + 2] = 1e-41f;
    sc.add_float_image(px);
    sc.add_record(STHIP_INSTANCE_TYPE_TRIANGLES, record(1, 1, 0));
    sc.add_record(STHIP_INSTANCE_TYPE_SPHERE, record(1, 0, 0xFFFFFFFFu));
    sc.add_medium(0.2f, 0, 0xFFFFFFFFu);
    analysis_case("infinities, a sphere and a medium", sc, true);
    const sthip::ImageRange r = sthip::scan_image_range(px.data(), 12, false);
    report("infinities and denormals are kept", r.hi[0] == inf && r.lo[1] == -inf && r.lo[2] == 1e-41f && r.nan_mask == 0);
  }
}

// (`code` and `message` by reference: the check that writes them is an argument of the same call)
static void refused(const char* name, bool ok, const int& code, int want_code, const std::string& message, const char* call, const char* want_text) {
  report(name, !ok && code == want_code && message.find(call) == 0 && message.find(want_text) != std::string::npos, message, true);
}

static void image_cases() {
  DeviceImage table[2];
  memset(table, 0, sizeof(table));
  table[0].w[0] = 4, table[0].h[0] = 3, table[0].levels = 1, table[0].format = STHIP_IMAGE_FORMAT_RGBA32F;
  table[1].w[0] = 8, table[1].h[0] = 2, table[1].levels = 1, table[1].format = STHIP_IMAGE_FORMAT_RGBA8_UNORM;
  DeviceImage1 masks[1] = {{0, 5, 7, STHIP_IMAGE_FORMAT_R8_UNORM}};
  sthip::ResidentImages scene;
  scene.has_scene = true;
  scene.images = table;
  scene.image_count = 2;
  scene.images1 = masks;
  scene.image1_count = 1;
  alignas(16) static float px[64];
  const uint32_t size = (uint32_t)sizeof(sthip_image_update);
  int code = 0;
  std::string msg;
  const char* call = "sthip_scene_set_images";
  auto entry = [&](uint32_t which, uint32_t index, const void* p, uint32_t w, uint32_t h, uint32_t dev) { return sthip_image_update{which, index, p, w, h, dev, 0}; };
  sthip_image_update good[3] = {entry(0, 0, px, 4, 3, 0), entry(0, 1, px, 8, 2, 1), entry(1, 0, px, 5, 7, 0)};
  report("three images of both arrays", sthip::check_images(scene, good, 3, size, code, msg), msg);
  report("no entries", sthip::check_images(scene, nullptr, 0, size, code, msg), msg);
  sthip::ResidentImages none;
  refused("no scene", sthip::check_images(none, good, 3, size, code, msg), code, STHIP_ERR_INVALID_ARGUMENT, msg, call, "no scene");
  refused("struct_size", sthip::check_images(scene, good, 3, size - 8, code, msg), code, STHIP_ERR_INVALID_ARGUMENT, msg, call, "struct_size");
  refused("NULL entries", sthip::check_images(scene, nullptr, 2, size, code, msg), code, STHIP_ERR_INVALID_ARGUMENT, msg, call, "entries is NULL");
  sthip_image_update e = entry(2, 0, px, 4, 3, 0);
  refused("which out of range", sthip::check_images(scene, &e, 1, size, code, msg), code, STHIP_ERR_INVALID_ARGUMENT, msg, call, "which");
  e = entry(0, 2, px, 4, 3, 0);
  refused("image index out of range", sthip::check_images(scene, &e, 1, size, code, msg), code, STHIP_ERR_INVALID_ARGUMENT, msg, call, "is not in gImages");
  e = entry(1, 1, px, 5, 7, 0);
  refused("mask index out of range", sthip::check_images(scene, &e, 1, size, code, msg), code, STHIP_ERR_INVALID_ARGUMENT, msg, call, "is not in gImage1s");
  e = entry(0, 0, nullptr, 4, 3, 0);
  refused("NULL pixels", sthip::check_images(scene, &e, 1, size, code, msg), code, STHIP_ERR_INVALID_ARGUMENT, msg, call, "pixels is NULL");
  e = entry(0, 0, px, 3, 4, 0);
  refused("differing extent", sthip::check_images(scene, &e, 1, size, code, msg), code, STHIP_ERR_INVALID_ARGUMENT, msg, call, "extent");
  e = entry(1, 0, px, 5, 6, 0);
  refused("differing mask extent", sthip::check_images(scene, &e, 1, size, code, msg), code, STHIP_ERR_INVALID_ARGUMENT, msg, call, "extent");
  sthip_image_update twice[3] = {good[0], good[2], good[0]};
  refused("the same image twice", sthip::check_images(scene, twice, 3, size, code, msg), code, STHIP_ERR_INVALID_ARGUMENT, msg, call, "named twice");
  sthip_image_update both[2] = {entry(0, 0, px, 4, 3, 0), entry(1, 0, px, 5, 7, 0)};
  report("index 0 of both arrays is two images", sthip::check_images(scene, both, 2, size, code, msg), msg);
  e = entry(0, 0, (const char*)px + 4, 4, 3, 1);
  refused("RGBA32F device pointer off 16 bytes", sthip::check_images(scene, &e, 1, size, code, msg), code, STHIP_ERR_INVALID_ARGUMENT, msg, call, "aligned to 16");
  e = entry(0, 0, (const char*)px + 4, 4, 3, 0);
  report("a host pointer need not be aligned", sthip::check_images(scene, &e, 1, size, code, msg), msg);
  e = entry(0, 1, (const char*)px + 4, 8, 2, 1);
  report("RGBA8 device pointer at 4 bytes", sthip::check_images(scene, &e, 1, size, code, msg), msg);
  e = entry(0, 1, (const char*)px + 2, 8, 2, 1);
  refused("RGBA8 device pointer off 4 bytes", sthip::check_images(scene, &e, 1, size, code, msg), code, STHIP_ERR_INVALID_ARGUMENT, msg, call, "aligned to 4");
  e = entry(1, 0, (const char*)px + 1, 5, 7, 1);
  refused("R8 device pointer off 4 bytes", sthip::check_images(scene, &e, 1, size, code, msg), code, STHIP_ERR_INVALID_ARGUMENT, msg, call, "aligned to 4");
}

static void material_data_cases() {
  Scene sc;
  sthip_MaterialRecord masked = record(0, 0.5f);
  masked.alpha_mask_index = 0;
  const uint32_t a0 = sc.add_record(STHIP_INSTANCE_TYPE_TRIANGLES, masked);
  sthip_MaterialRecord light = record(0, 0.5f);
  light.values[0].value[3] = 5.0f;  // emission
  const uint32_t a1 = sc.add_record(STHIP_INSTANCE_TYPE_TRIANGLES, light);
  const uint32_t a2 = sc.add_medium(0.1f, 1, 0xFFFFFFFFu);
  const uint32_t a3 = sc.add_record(STHIP_INSTANCE_TYPE_SPHERE, record(0, 0.5f));
  std::vector<sthip::MaterialInstance> inst;
  for (const sthip_InstanceData& i : sc.instances) inst.push_back(sthip::MaterialInstance{i.packed[0] >> 4, i.packed[0] & 0xFu});
  sthip::ResidentMaterials scene;
  scene.has_scene = true;
  scene.materials = sc.materials.data();
  scene.material_bytes = sc.materials.size();
  scene.instances = inst.data();
  scene.instance_count = (uint32_t)inst.size();
  scene.image_count = 2;
  scene.image1_count = 1;
  scene.volume_count = 2;
  const char* call = "sthip_scene_set_material_data";
  int code = 0;
  std::string msg;
  std::vector<uint8_t> edited;
  const float colour[3] = {0.9f, 0.1f, 0.2f};
  bool ok = sthip::check_material_data(scene, a0, colour, 12, edited, code, msg);
  report("a colour edit", ok && edited.size() == sc.materials.size() && !memcmp(edited.data() + a0, colour, 12) && !memcmp(edited.data() + a0 + 12, sc.materials.data() + a0 + 12, sc.materials.size() - a0 - 12), msg);
  const uint32_t one = 1;
  report("a record starts binding an image", sthip::check_material_data(scene, a0 + 16, &one, 4, edited, code, msg), msg);
  report("an empty range", sthip::check_material_data(scene, 8, nullptr, 0, edited, code, msg) && edited == sc.materials, msg);
  const float strength = 9.0f, zero = 0.0f, g = 0.9f;
  report("a light's strength", sthip::check_material_data(scene, a1 + 12, &strength, 4, edited, code, msg), msg);
  report("a medium's anisotropy", sthip::check_material_data(scene, a2 + 12, &g, 4, edited, code, msg), msg);
  report("the whole buffer as it is", sthip::check_material_data(scene, 0, sc.materials.data(), (uint32_t)sc.materials.size(), edited, code, msg), msg);
  sthip::ResidentMaterials none;
  refused("no scene", sthip::check_material_data(none, 0, colour, 12, edited, code, msg), code, STHIP_ERR_INVALID_ARGUMENT, msg, call, "no scene");
  refused("NULL data", sthip::check_material_data(scene, 0, nullptr, 12, edited, code, msg), code, STHIP_ERR_INVALID_ARGUMENT, msg, call, "data is NULL");
  refused("unaligned offset", sthip::check_material_data(scene, 2, colour, 12, edited, code, msg), code, STHIP_ERR_INVALID_ARGUMENT, msg, call, "multiples of 4");
  refused("unaligned size", sthip::check_material_data(scene, 0, colour, 6, edited, code, msg), code, STHIP_ERR_INVALID_ARGUMENT, msg, call, "multiples of 4");
  refused("range past the end", sthip::check_material_data(scene, (uint32_t)sc.materials.size() - 8, colour, 12, edited, code, msg), code, STHIP_ERR_INVALID_ARGUMENT, msg, call, "ends past");
  const uint32_t two = 2, no_image = 0xFFFFFFFFu;
  refused("image index out of range", sthip::check_material_data(scene, a0 + 16, &two, 4, edited, code, msg), code, STHIP_ERR_INVALID_ARGUMENT, msg, call, "not in gImages");
  refused("bump index out of range", sthip::check_material_data(scene, a0 + 64, &two, 4, edited, code, msg), code, STHIP_ERR_INVALID_ARGUMENT, msg, call, "bump map");
  refused("mask index out of range", sthip::check_material_data(scene, a0 + 60, &one, 4, edited, code, msg), code, STHIP_ERR_INVALID_ARGUMENT, msg, call, "not in gImage1s");
  refused("volume index out of range", sthip::check_material_data(scene, a2 + 32, &two, 4, edited, code, msg), code, STHIP_ERR_INVALID_ARGUMENT, msg, call, "not in gVolumes");
  refused("a triangle instance loses its mask", sthip::check_material_data(scene, a0 + 60, &no_image, 4, edited, code, msg), code, STHIP_ERR_UNSUPPORTED, msg, call, "alpha_mask_index");
  const uint32_t zero_index = 0;
  refused("a triangle instance gains a mask", sthip::check_material_data(scene, a1 + 60, &zero_index, 4, edited, code, msg), code, STHIP_ERR_UNSUPPORTED, msg, call, "alpha_mask_index");
  report("a sphere's mask index is nobody's business", sthip::check_material_data(scene, a3 + 60, &zero_index, 4, edited, code, msg), msg);
  refused("a medium's volume changes", sthip::check_material_data(scene, a2 + 32, &zero_index, 4, edited, code, msg), code, STHIP_ERR_UNSUPPORTED, msg, call, "volume indices");
  refused("a light goes out", sthip::check_material_data(scene, a1 + 12, &zero, 4, edited, code, msg), code, STHIP_ERR_UNSUPPORTED, msg, call, "emission");
  refused("a surface starts to emit", sthip::check_material_data(scene, a3 + 12, &strength, 4, edited, code, msg), code, STHIP_ERR_UNSUPPORTED, msg, call, "emission");
  // a refused call leaves the caller's buffer alone
  report("the resident bytes are never written", !memcmp(sc.materials.data() + a1 + 12, &light.values[0].value[3], 4));
}

int main() {
  analysis_cases();
  image_cases();
  material_data_cases();
  if (failures) {
    std::printf("%d FAILED\n", failures);
    return 1;
  }
  std::printf("MATERIAL UPDATE CHECK OK\n");
  return 0;
}
