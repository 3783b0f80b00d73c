// scene_prepare_check.cpp — the host part of sthip_scene_upload (stratum_amd/csrc/scene_prepare.cpp) as a plain CPU program,
// so that it runs under AddressSanitizer / UndefinedBehaviorSanitizer. Reads the scene arrays tests/test_host_cpp.py dumps:
//   <dir>/{vertices,indices,instances,xf,inv_xf,materials,lights,distributions}.bin  raw arrays
//   <dir>/images.bin, masks.bin   u32 count, then per image u32 width, height, format, u64 payload bytes, payload
//   <dir>/volumes.bin             u32 count, then per grid u64 bytes as the descriptor states them, u64 payload bytes, payload
// Two modes:
//   scene_prepare_check check <dir> [null:<array> ...]   check_scene with the named arrays NULL (their counts stay); prints
//                                                        "ACCEPTED", or "REFUSED <code>" and the message on the next line
//   scene_prepare_check results <dir>                    every result of the unit against <dir>/expect_<name>.bin (the numpy
//                                                        restatement of the Python test), byte for byte, where that file exists
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../stratum_amd/csrc/scene_prepare.h"

namespace sthip {  // the GPU builder's entry points are never reached with the SAH builder; defined to satisfy the linker
bool lbvh_build_gpu(const std::vector<BvhTri>&, std::vector<BvhNode>&, std::vector<BvhTri>&, uint32_t&, uint32_t&, float&, std::string& err) {
  err = "no device in this harness";
  return false;
}
bool lbvh_build_device(const DeviceBuildTarget&, const std::vector<MeshPiece>&, uint32_t, uint32_t, uint32_t&, uint32_t&, float*, float&, std::string& err, std::vector<FrontierEntry>*, uint32_t) {
  err = "no device in this harness";
  return false;
}
}  // namespace sthip

static bool slurp_bytes(const std::string& path, std::vector<uint8_t>& v) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) return false;
  v.resize((size_t)f.tellg());
  f.seekg(0);
  f.read((char*)v.data(), v.size());
  return true;
}
template <typename T>
static std::vector<T> slurp(const std::string& path) {
  std::vector<uint8_t> b;
  if (!slurp_bytes(path, b)) {
    std::fprintf(stderr, "cannot open %s\n", path.c_str());
    std::exit(2);
  }
  std::vector<T> v(b.size() / sizeof(T));
  if (!v.empty()) memcpy(v.data(), b.data(), v.size() * sizeof(T));
  return v;
}
template <typename T>
static T take(const std::vector<uint8_t>& b, size_t& at) {
  T v;
  if (at + sizeof(T) > b.size()) std::exit(2);
  memcpy(&v, b.data() + at, sizeof(T));
  at += sizeof(T);
  return v;
}

struct Scene {
  std::vector<sthip_PackedVertexData> vertices;
  std::vector<uint8_t> indices, materials;
  std::vector<sthip_InstanceData> instances;
  std::vector<sthip_TransformData> xf, inv;
  std::vector<uint32_t> lights;
  std::vector<float> distributions;
  std::vector<std::vector<float>> payloads;  // (float storage: the payload of a float image is read through a float pointer)
  std::vector<sthip_image_desc> images, masks;
  std::vector<uint8_t> image_formats, mask_formats;
  std::vector<sthip_volume_desc> volumes;
  sthip_scene_desc d{};

  void images_from(const std::string& path, std::vector<sthip_image_desc>& out, std::vector<uint8_t>& formats) {
    const std::vector<uint8_t> b = slurp<uint8_t>(path);
    size_t at = 0;
    const uint32_t n = take<uint32_t>(b, at);
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t w = take<uint32_t>(b, at), h = take<uint32_t>(b, at), format = take<uint32_t>(b, at);
      const uint64_t bytes = take<uint64_t>(b, at);
      if (at + bytes > b.size()) std::exit(2);
      payloads.emplace_back((bytes + 3) / 4);
      if (bytes) memcpy(payloads.back().data(), b.data() + at, bytes);
      at += bytes;
      out.push_back(sthip_image_desc{bytes ? payloads.back().data() : nullptr, w, h});
      formats.push_back((uint8_t)format);
    }
  }
  explicit Scene(const std::string& dir) {
    vertices = slurp<sthip_PackedVertexData>(dir + "/vertices.bin");
    indices = slurp<uint8_t>(dir + "/indices.bin");
    instances = slurp<sthip_InstanceData>(dir + "/instances.bin");
    xf = slurp<sthip_TransformData>(dir + "/xf.bin");
    inv = slurp<sthip_TransformData>(dir + "/inv_xf.bin");
    materials = slurp<uint8_t>(dir + "/materials.bin");
    lights = slurp<uint32_t>(dir + "/lights.bin");
    distributions = slurp<float>(dir + "/distributions.bin");
    images_from(dir + "/images.bin", images, image_formats);
    images_from(dir + "/masks.bin", masks, mask_formats);
    {
      const std::vector<uint8_t> b = slurp<uint8_t>(dir + "/volumes.bin");
      size_t at = 0;
      const uint32_t n = take<uint32_t>(b, at);
      for (uint32_t i = 0; i < n; i++) {
        const uint64_t stated = take<uint64_t>(b, at), bytes = take<uint64_t>(b, at);
        if (at + bytes > b.size()) std::exit(2);
        payloads.emplace_back((bytes + 3) / 4);
        if (bytes) memcpy(payloads.back().data(), b.data() + at, bytes);
        at += bytes;
        volumes.push_back(sthip_volume_desc{payloads.back().data(), stated});
      }
    }
    const size_t indices_bytes = indices.size();
    indices.resize(indices_bytes + 8, 0);
    d.gVertices = vertices.data();
    d.vertex_count = (uint32_t)vertices.size();
    d.gIndices = indices.data();
    d.indices_bytes = (uint32_t)indices_bytes;
    d.gInstances = instances.data();
    d.instance_count = (uint32_t)instances.size();
    d.gInstanceTransforms = xf.data();
    d.gInstanceInverseTransforms = inv.data();
    d.gMaterialData = materials.data();
    d.material_bytes = (uint32_t)materials.size();
    d.gLightInstances = lights.data();
    d.light_count = (uint32_t)lights.size();
    d.gImages = images.data();
    d.image_count = (uint32_t)images.size();
    d.gDistributions = distributions.data();
    d.distribution_count = (uint32_t)distributions.size();
    d.gImage1s = masks.data();
    d.image1_count = (uint32_t)masks.size();
    d.gVolumes = volumes.data();
    d.volume_count = (uint32_t)volumes.size();
  }
};

static int failures = 0;
// `got` against <dir>/expect_<name>.bin, where the Python side wrote one
static void expect(const std::string& dir, const char* name, const void* got, size_t bytes) {
  std::vector<uint8_t> want;
  if (!slurp_bytes(dir + "/expect_" + name + ".bin", want)) return;
  if (want.size() != bytes) {
    std::printf("FAIL: %s has %zu bytes, expected %zu\n", name, bytes, want.size());
    failures++;
    return;
  }
  for (size_t i = 0; i < bytes; i++)
    if (((const uint8_t*)got)[i] != want[i]) {
      std::printf("FAIL: %s differs at byte %zu (%u, expected %u)\n", name, i, ((const uint8_t*)got)[i], want[i]);
      failures++;
      return;
    }
  std::printf("%s: %zu bytes agree\n", name, bytes);
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string mode = argv[1], dir = argv[2];
  Scene sc(dir);
  sthip_scene_desc& d = sc.d;
  const uint8_t* formats = sc.image_formats.empty() ? nullptr : sc.image_formats.data();
  const uint8_t* formats1 = sc.mask_formats.empty() ? nullptr : sc.mask_formats.data();
  if (mode == "check") {
    bool no_scene = false;
    for (int i = 3; i < argc; i++) {
      const std::string a = argv[i];
      if (a == "null:scene") no_scene = true;
      else if (a == "null:gVertices") d.gVertices = nullptr;
      else if (a == "null:gIndices") d.gIndices = nullptr;
      else if (a == "null:gInstances") d.gInstances = nullptr;
      else if (a == "null:gInstanceTransforms") d.gInstanceTransforms = nullptr;
      else if (a == "null:gInstanceInverseTransforms") d.gInstanceInverseTransforms = nullptr;
      else if (a == "null:gMaterialData") d.gMaterialData = nullptr;
      else if (a == "null:gLightInstances") d.gLightInstances = nullptr;
      else if (a == "null:gImages") d.gImages = nullptr;
      else if (a == "null:gImage1s") d.gImage1s = nullptr;
      else if (a == "null:gDistributions") d.gDistributions = nullptr;
      else if (a == "null:gVolumes") d.gVolumes = nullptr;
      else return std::fprintf(stderr, "unknown argument %s\n", a.c_str()), 2;
    }
    int code = 0;
    std::string message;
    if (sthip::check_scene(no_scene ? nullptr : &d, formats, formats1, code, message)) std::printf("ACCEPTED\n");
    else std::printf("REFUSED %d\n%s\n", code, message.c_str());
    return 0;
  }
  if (mode != "results") return 2;
  int code = 0;
  std::string message;
  if (!sthip::check_scene(&d, formats, formats1, code, message)) return std::printf("FAIL: refused (%d): %s\n", code, message.c_str()), 1;
  const sthip::MaterialAnalysis m = sthip::analyse_materials(d, formats);
  const uint8_t flags[5] = {m.has_specular, m.textured, m.any_alpha, m.has_spheres, m.has_volumes};
  expect(dir, "scene_flags", flags, sizeof(flags));
  expect(dir, "inst_flags", m.inst_flags.data(), m.inst_flags.size());
  expect(dir, "instance_is_volume", m.instance_is_volume.data(), m.instance_is_volume.size());
  expect(dir, "volume_instances", &m.volume_instances, 4);
  const sthip::ImageLayout images = sthip::layout_images(d, formats);
  if (images.error) return std::printf("FAIL: %s\n", images.error), 1;
  const uint64_t words8 = images.texels8;
  expect(dir, "image_table", images.table.data(), images.table.size() * sizeof(DeviceImage));
  expect(dir, "image_texels", images.texels.data(), images.texels.size() * sizeof(float));
  expect(dir, "image_words8", &words8, 8);
  const sthip::MaskLayout masks = sthip::layout_alpha_masks(d, formats1);
  if (masks.error) return std::printf("FAIL: %s\n", masks.error), 1;
  expect(dir, "mask_table", masks.table.data(), masks.table.size() * sizeof(DeviceImage1));
  expect(dir, "mask_texels", masks.texels.data(), masks.texels.size() * sizeof(float));
  expect(dir, "mask_texels8", masks.texels8.data(), masks.texels8.size());
  std::vector<uint32_t> first_words;
  const uint64_t words = sthip::volume_first_words(d, first_words);
  expect(dir, "volume_first_words", first_words.data(), first_words.size() * 4);
  expect(dir, "volume_words", &words, 8);
  {  // the emitter boxes read gIndices where only the builder validates them: after a build, as the upload calls it
    sthip::BuiltBvh built;
    std::string err;
    if (!sthip::build_scene_bvh(d, built, err, sthip::BVH_BUILDER_SAH_HOST, nullptr, false)) return std::printf("BUILD FAILED: %s\n", err.c_str()), 1;
    std::vector<EmitterBounds> bounds;
    sthip::emitter_bounds(d, m.inst_flags, bounds);
    const uint32_t count = (uint32_t)bounds.size();
    expect(dir, "emitter_count", &count, 4);
    expect(dir, "emitters", bounds.data(), bounds.size() * sizeof(EmitterBounds));
  }
  if (failures) return 1;
  std::printf("SCENE PREPARE OK\n");
  return 0;
}
