// environment_check.cpp — the host part of sthip_scene_set_environment (stratum_amd/csrc/scene_prepare.cpp: check_environment,
// environment_row_sines) as a plain CPU program with its own main: built with -fsanitize=address,undefined and run directly
// (tests/test_environment.py). A resident scene is stated by hand — gMaterialData with one material record that names image 1,
// an image environment record over image 0 (8 x 4, RGBA32F), a constant environment record, an environment over the 8-bit
// image 2 and one over the material's image 1 — and every refusal of include/sthip.h must return its code and say why, every
// accepted description must pass with the plan it implies. Prints one line per case and "ENVIRONMENT CHECK OK" at the end.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../stratum_amd/csrc/scene_prepare.h"

static int failures = 0;

struct Resident {
  std::vector<uint8_t> materials;
  std::vector<DeviceImage> images;
  std::vector<uint8_t> in_material;
  uint32_t distribution_count = 0;
  bool has_scene = true;
  sthip::ResidentEnvironmentScene view() const {
    sthip::ResidentEnvironmentScene r;
    r.has_scene = has_scene;
    r.materials = materials.data();
    r.material_bytes = materials.size();
    r.images = images.data();
    r.image_count = (uint32_t)images.size();
    r.image_in_material = in_material.data();
    r.distribution_count = distribution_count;
    return r;
  }
};

static uint32_t append_record(std::vector<uint8_t>& m, const float value[3], uint32_t image, const uint32_t* tables) {
  const uint32_t at = (uint32_t)m.size();
  m.resize(at + (tables ? 32 : 16));
  memcpy(m.data() + at, value, 12);
  memcpy(m.data() + at + 12, &image, 4);
  if (tables) memcpy(m.data() + at + 16, tables, 16);
  return at;
}

static DeviceImage image_of(uint32_t w, uint32_t h, uint32_t format) {
  DeviceImage im;
  memset(&im, 0, sizeof(im));
  im.w[0] = (uint16_t)w, im.h[0] = (uint16_t)h, im.levels = 1, im.format = format;
  return im;
}

static void expect(const char* name, const Resident& r, const sthip_environment_desc* d, int want_code, const char* want_text, const sthip::EnvironmentPlan* want_plan = nullptr) {
  sthip::EnvironmentPlan plan;
  int code = 0;
  std::string message;
  const bool ok = sthip::check_environment(r.view(), d, plan, code, message);
  bool pass;
  if (want_code == STHIP_OK) {
    pass = ok;
    if (pass && want_plan)
      pass = plan.has_image == want_plan->has_image && plan.replace_pixels == want_plan->replace_pixels && plan.build_tables == want_plan->build_tables && plan.set_value == want_plan->set_value &&
             (!plan.has_image || (plan.image_index == want_plan->image_index && plan.width == want_plan->width && plan.height == want_plan->height && !memcmp(plan.table, want_plan->table, 16)));
  } else {
    pass = !ok && code == want_code && message.find("sthip_scene_set_environment") == 0 && message.find(want_text) != std::string::npos;
  }
  std::printf("%s %s: %s\n", pass ? "ok  " : "FAIL", name, ok ? "ACCEPTED" : ("REFUSED " + std::to_string(code) + " " + message).c_str());
  if (!pass) failures++;
}

int main() {
  const uint32_t W = 8, H = 4;
  const uint32_t tables[4] = {0, H, H + H * W, H + H * W + H + 1};  // back to back, as the hosts lay them out
  const uint32_t table_floats = H + H * W + (H + 1) + H * (W + 1);
  Resident r;
  {  // one material record (sthip_MaterialRecord) whose first value names image 1
    sthip_MaterialRecord rec;
    memset(&rec, 0, sizeof(rec));
    for (int k = 0; k < 3; k++) rec.values[k].image_index = 0xFFFFFFFFu;
    rec.values[0].image_index = 1;
    rec.bump_index = rec.alpha_mask_index = 0xFFFFFFFFu;
    r.materials.resize(sizeof(rec));
    memcpy(r.materials.data(), &rec, sizeof(rec));
  }
  const float one[3] = {1, 1, 1};
  const uint32_t env = append_record(r.materials, one, 0, tables);
  const uint32_t constant = append_record(r.materials, one, 0xFFFFFFFFu, nullptr);
  const uint32_t env8 = append_record(r.materials, one, 2, tables);
  const uint32_t env_shared = append_record(r.materials, one, 1, tables);
  const uint32_t overlap_tables[4] = {0, H - 1, H + H * W, H + H * W + H + 1};
  const uint32_t env_overlap = append_record(r.materials, one, 0, overlap_tables);
  const uint32_t far_tables[4] = {0, H, H + H * W, H + H * W + H + 2};
  const uint32_t env_outside = append_record(r.materials, one, 0, far_tables);
  const uint32_t env_no_image = append_record(r.materials, one, 7, tables);
  r.images = {image_of(W, H, STHIP_IMAGE_FORMAT_RGBA32F), image_of(W, H, STHIP_IMAGE_FORMAT_RGBA32F), image_of(W, H, STHIP_IMAGE_FORMAT_RGBA8_UNORM)};
  r.in_material = {0, 1, 0};
  r.distribution_count = table_floats;

  std::vector<float> pixels((size_t)W * H * 4, 0.5f);
  const float value[3] = {0.5f, 2.0f, 0.25f}, zero[3] = {0, 0, 0}, negative_zero[3] = {-0.0f, 0, 0};
  auto desc = [&](uint32_t address, const float* v, const void* px, uint32_t w = 8, uint32_t h = 4, uint32_t device = 0) {
    sthip_environment_desc d{};
    d.struct_size = sizeof(d);
    d.material_address = address;
    d.value = v;
    d.pixels = px;
    d.width = px ? w : 0;
    d.height = px ? h : 0;
    d.device_ptr = device;
    return d;
  };
  sthip::EnvironmentPlan want;
  want.has_image = true, want.image_index = 0, want.width = W, want.height = H;
  memcpy(want.table, tables, 16);

  // ---- accepted ----
  sthip_environment_desc d = desc(env, nullptr, pixels.data());
  want.replace_pixels = true, want.build_tables = true, want.set_value = false;
  expect("pixels", r, &d, STHIP_OK, "", &want);
  d = desc(env, value, pixels.data(), W, H, 1);
  want.set_value = true;
  expect("pixels and value, device pointer", r, &d, STHIP_OK, "", &want);
  d = desc(env, nullptr, nullptr);
  want.replace_pixels = false, want.build_tables = true, want.set_value = false;
  expect("tables only", r, &d, STHIP_OK, "", &want);
  d = desc(env, value, nullptr);
  want.build_tables = false, want.set_value = true;
  expect("value only", r, &d, STHIP_OK, "", &want);
  {
    sthip::EnvironmentPlan c;
    c.set_value = true;
    d = desc(constant, value, nullptr);
    expect("value of a constant environment", r, &d, STHIP_OK, "", &c);
    c.set_value = false;
    d = desc(constant, nullptr, nullptr);
    expect("nothing to do for a constant environment", r, &d, STHIP_OK, "", &c);
  }
  d = desc(env_shared, value, nullptr);
  {
    sthip::EnvironmentPlan s = want;
    s.image_index = 1;
    expect("value of an environment whose image a material shares", r, &d, STHIP_OK, "", &s);
    s.build_tables = true, s.set_value = false;
    d = desc(env_shared, nullptr, nullptr);
    expect("tables of an environment whose image a material shares", r, &d, STHIP_OK, "", &s);
  }

  // ---- refused: STHIP_ERR_INVALID_ARGUMENT ----
  const int bad = STHIP_ERR_INVALID_ARGUMENT;
  expect("NULL description", r, nullptr, bad, "NULL");
  {
    Resident none = r;
    none.has_scene = false;
    d = desc(env, value, nullptr);
    expect("no scene", none, &d, bad, "no scene");
  }
  d = desc(env, value, nullptr);
  d.struct_size = sizeof(d) - 8;
  expect("struct_size", r, &d, bad, "struct_size");
  d = desc(env + 2, value, nullptr);
  expect("unaligned address", r, &d, bad, "material_address");
  d = desc((uint32_t)r.materials.size() - 12, value, nullptr);
  expect("address whose record runs past gMaterialData", r, &d, bad, "material_address");
  d = desc(0xFFFFFFF0u, value, nullptr);
  expect("address far outside", r, &d, bad, "material_address");
  d = desc(constant, nullptr, pixels.data());
  expect("pixels for a record without an image", r, &d, bad, "without an image");
  d = desc(env_no_image, nullptr, nullptr);
  expect("image index not in gImages", r, &d, bad, "not in gImages");
  d = desc(env, nullptr, pixels.data(), W + 1, H);
  expect("wrong width", r, &d, bad, "extent");
  d = desc(env, nullptr, pixels.data(), H, W);
  expect("transposed extent", r, &d, bad, "extent");
  d = desc(env_outside, nullptr, nullptr);
  expect("table outside gDistributions", r, &d, bad, "outside gDistributions");
  {
    Resident shorter = r;
    shorter.distribution_count = table_floats - 1;
    d = desc(env, value, nullptr);
    expect("gDistributions one float short", shorter, &d, bad, "outside gDistributions");
  }
  d = desc(env_overlap, nullptr, nullptr);
  expect("overlapping tables", r, &d, bad, "overlap");
  d = desc(env, zero, nullptr);
  expect("zero value", r, &d, bad, "zero");
  d = desc(env, negative_zero, pixels.data());
  expect("zero value (negative zero) with pixels", r, &d, bad, "zero");
  d = desc(constant, zero, nullptr);
  expect("zero value of a constant environment", r, &d, bad, "zero");

  // ---- refused: STHIP_ERR_UNSUPPORTED ----
  d = desc(env8, nullptr, pixels.data());
  expect("8-bit environment, pixels", r, &d, STHIP_ERR_UNSUPPORTED, "8-bit");
  d = desc(env8, nullptr, nullptr);
  expect("8-bit environment, tables", r, &d, STHIP_ERR_UNSUPPORTED, "8-bit");
  d = desc(env_shared, nullptr, pixels.data());
  expect("pixels for an image a material names", r, &d, STHIP_ERR_UNSUPPORTED, "material record");

  // ---- the sines the device is sent ----
  for (uint32_t h : {1u, 2u, 3u, 130u, 65535u}) {
    std::vector<double> s;
    sthip::environment_row_sines(h, s);
    bool ok = s.size() == h;
    const float inv = 1 / (float)h;
    for (uint32_t y = 0; ok && y < h; y++) ok = s[y] == std::sin(M_PI * (y + 0.5f) * inv) && s[y] > 0 && s[y] <= 1;
    std::printf("%s sines of %u rows\n", ok ? "ok  " : "FAIL", h);
    if (!ok) failures++;
  }
  if (failures) return std::printf("%d FAILED\n", failures), 1;
  std::printf("ENVIRONMENT CHECK OK\n");
  return 0;
}
