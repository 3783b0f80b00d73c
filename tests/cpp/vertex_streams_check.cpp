// vertex_streams_check.cpp — the host part of sthip_scene_set_vertices (stratum_amd/csrc/scene_prepare.cpp:
// check_vertex_streams, list_vertex_meshes) as a plain CPU program with its own main: built with -fsanitize=address,undefined
// and run directly (tests/test_vertex_streams.py). Every refusal of include/sthip.h must return STHIP_ERR_INVALID_ARGUMENT and
// name the field, every accepted description must pass; the mesh list of a hand-made instance table must come out in the
// order of the normal contract. Prints one line per case and "VERTEX STREAMS CHECK OK" at the end.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../stratum_amd/csrc/scene_prepare.h"

static int failures = 0;

static void expect(const char* name, bool has_scene, uint32_t scene_vertices, const sthip_vertex_streams* d, int want_code, const char* want_text) {
  int code = 0;
  std::string message;
  const bool ok = sthip::check_vertex_streams(has_scene, scene_vertices, d, code, message);
  const bool pass = want_code == STHIP_OK ? ok : (!ok && code == want_code && message.find("sthip_scene_set_vertices") == 0 && message.find(want_text) != std::string::npos);
  std::printf("%s %s: %s\n", pass ? "ok  " : "FAIL", name, ok ? "ACCEPTED" : ("REFUSED " + std::to_string(code) + " " + message).c_str());
  if (!pass) failures++;
}

// make_instance_triangles, scene.h:51-61
static sthip_InstanceData triangles(uint32_t indices_byte_offset, uint32_t first_vertex, uint32_t stride, uint32_t prims, uint32_t material = 0) {
  sthip_InstanceData d;
  d.packed[0] = STHIP_INSTANCE_TYPE_TRIANGLES | (material << 4);
  d.packed[1] = 0xFFFu | (prims << 12) | (stride << 28);
  d.packed[2] = first_vertex;
  d.packed[3] = indices_byte_offset;
  return d;
}

static void expect_meshes(const char* name, const std::vector<sthip_InstanceData>& instances, const std::vector<sthip::VertexMesh>& want) {
  const std::vector<sthip::VertexMesh> got = sthip::list_vertex_meshes(instances.data(), (uint32_t)instances.size());
  bool pass = got.size() == want.size();
  for (size_t k = 0; pass && k < got.size(); k++)
    pass = got[k].indices_byte_offset == want[k].indices_byte_offset && got[k].first_vertex == want[k].first_vertex && got[k].index_stride == want[k].index_stride && got[k].prim_count == want[k].prim_count;
  std::printf("%s %s: %zu meshes\n", pass ? "ok  " : "FAIL", name, got.size());
  if (!pass) failures++;
}

int main() {
  const int BAD = STHIP_ERR_INVALID_ARGUMENT;
  alignas(16) static float storage[64];
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(storage);
  sthip_vertex_streams good{};
  good.struct_size = sizeof(good);
  good.first_vertex = 3;
  good.vertex_count = 5;
  good.position_stride = 12;
  good.positions = storage;

  // ---- refusals ----
  expect("no scene", false, 8, &good, BAD, "no scene is resident");
  expect("NULL description", true, 8, nullptr, BAD, "description is NULL");
  {
    sthip_vertex_streams d = good;
    d.struct_size = sizeof(d) - 8;
    expect("struct_size", true, 8, &d, BAD, "struct_size");
    d.struct_size = 0;
    expect("struct_size zero", true, 8, &d, BAD, "struct_size");
  }
  {
    sthip_vertex_streams d = good;
    d.positions = nullptr;
    expect("NULL positions", true, 8, &d, BAD, "positions is NULL");
    d.vertex_count = 0;
    expect("NULL positions, empty range", true, 8, &d, BAD, "positions is NULL");
  }
  {
    sthip_vertex_streams d = good;
    d.vertex_count = 6;
    expect("range past vertex_count", true, 8, &d, BAD, "first_vertex + vertex_count");
    d.first_vertex = 0xFFFFFFFFu, d.vertex_count = 2;  // (the sum does not wrap)
    expect("range that wraps", true, 8, &d, BAD, "first_vertex + vertex_count");
    d.first_vertex = 9, d.vertex_count = 0;
    expect("empty range past the end", true, 8, &d, BAD, "first_vertex + vertex_count");
  }
  {
    sthip_vertex_streams d = good;
    d.positions = bytes + 2;
    expect("positions unaligned", true, 8, &d, BAD, "positions is not 4-byte aligned");
    d = good;
    d.normals = bytes + 1, d.normal_stride = 12;
    expect("normals unaligned", true, 8, &d, BAD, "normals is not 4-byte aligned");
    d = good;
    d.texcoords = bytes + 3, d.texcoord_stride = 8;
    expect("texcoords unaligned", true, 8, &d, BAD, "texcoords is not 4-byte aligned");
    d = good;
    d.position_stride = 14;
    expect("position_stride not a multiple of 4", true, 8, &d, BAD, "position_stride");
    d = good;
    d.normals = storage, d.normal_stride = 18;
    expect("normal_stride not a multiple of 4", true, 8, &d, BAD, "normal_stride");
    d = good;
    d.texcoords = storage, d.texcoord_stride = 10;
    expect("texcoord_stride not a multiple of 4", true, 8, &d, BAD, "texcoord_stride");
  }
  {
    sthip_vertex_streams d = good;
    d.position_stride = 8;
    expect("position_stride below 12", true, 8, &d, BAD, "position_stride");
    d.position_stride = 0;
    expect("position_stride zero", true, 8, &d, BAD, "position_stride");
    d = good;
    d.normals = storage, d.normal_stride = 8;
    expect("normal_stride below 12", true, 8, &d, BAD, "normal_stride");
    d = good;
    d.texcoords = storage, d.texcoord_stride = 4;
    expect("texcoord_stride below 8", true, 8, &d, BAD, "texcoord_stride");
  }
  {
    sthip_vertex_streams d = good;
    d.normals = storage, d.normal_stride = 12, d.recompute_normals = 1;
    expect("normals with recompute_normals", true, 8, &d, BAD, "recompute_normals");
  }

  // ---- accepted ----
  expect("positions only", true, 8, &good, STHIP_OK, "");
  {
    sthip_vertex_streams d = good;
    d.vertex_count = 0;
    expect("empty range", true, 8, &d, STHIP_OK, "");
    d.first_vertex = 8;
    expect("empty range at the end", true, 8, &d, STHIP_OK, "");
    d = good;
    d.struct_size = sizeof(d) + 16;  // (a later, longer struct)
    expect("larger struct_size", true, 8, &d, STHIP_OK, "");
    d = good;
    d.normal_stride = 7, d.texcoord_stride = 2;  // (strides of absent streams are not read)
    expect("strides of absent streams", true, 8, &d, STHIP_OK, "");
    d = good;
    d.positions = bytes + 4, d.position_stride = 20;  // 4- but not 8-byte aligned
    d.normals = bytes + 12, d.normal_stride = 32;
    d.texcoords = bytes + 8, d.texcoord_stride = 8;
    expect("all streams, 4-byte alignment", true, 8, &d, STHIP_OK, "");
    d = good;
    d.recompute_normals = 1;
    expect("recompute_normals", true, 8, &d, STHIP_OK, "");
    d.device_ptr = 1;
    expect("device_ptr", true, 8, &d, STHIP_OK, "");
  }

  // ---- the mesh list ----
  {
    std::vector<sthip_InstanceData> in;
    in.push_back(triangles(400, 50, 4, 7));       // the last mesh comes first
    in.push_back(triangles(0, 0, 2, 3, 9));       // 16-bit: 18 bytes, so the next mesh starts at 20 (aligned up to 4)
    in.push_back(triangles(20, 4, 4, 2));
    in.push_back(triangles(0, 0, 2, 3, 5));       // shares the tuple of the second (another material): counted once
    in.push_back(triangles(20, 4, 4, 2));         // ... and the third
    in.push_back(triangles(20, 4, 2, 2));         // same offset and first vertex, another stride: a mesh of its own, before stride 4
    in.push_back(triangles(20, 4, 4, 1));         // same but fewer triangles: before the one with 2
    in.push_back(triangles(20, 2, 4, 9));         // same offset, a lower first vertex: before all of them
    sthip_InstanceData sphere{};
    sphere.packed[0] = STHIP_INSTANCE_TYPE_SPHERE;
    sphere.packed[2] = 0x3F800000u;
    in.insert(in.begin() + 2, sphere);            // spheres and volumes have no mesh
    sthip_InstanceData volume{};
    volume.packed[0] = STHIP_INSTANCE_TYPE_VOLUME;
    in.push_back(volume);
    expect_meshes("order, shared tuples, strides, aligned offset", in, {{0, 0, 2, 3}, {20, 2, 4, 9}, {20, 4, 2, 2}, {20, 4, 4, 1}, {20, 4, 4, 2}, {400, 50, 4, 7}});
    expect_meshes("no instances", {}, {});
    expect_meshes("spheres only", {sphere, sphere}, {});
    const std::vector<sthip::VertexMesh> none = sthip::list_vertex_meshes(nullptr, 0);
    if (!none.empty()) failures++;
  }
  if (failures) {
    std::printf("%d FAILED\n", failures);
    return 1;
  }
  std::printf("VERTEX STREAMS CHECK OK\n");
  return 0;
}
