// top_level_ref.cpp — the reference of the device-built top level's entry boxes (tests/test_top_level.py): the HOST builder,
// sthip::rebuild_top_level (stratum_amd/csrc/bvh_build.cpp), as a plain CPU program.
//   top_level_ref <dir> <case>...
// <dir>/{vertices,indices,instances,xf,inv_xf,materials}.bin are the raw scene arrays, <dir>/volume<k>.bin the NanoVDB grids
// of gVolumes; every <case> names <dir>/<case>_xf.bin and <dir>/<case>_inv.bin, the moved matrices. The scene is built once
// (binned SAH, as an upload does), then for every case the top level is rebuilt and <dir>/<case>_ref.bin is written:
// uint32 entry count, 6 floats per entry (lo, hi: the exact boxes, read from the leaf slots of the top-level nodes, or the
// merged mesh's box where there is no top level), centre.xyz, radius, uint32 node count, uint32 top_is_world_blas.
// The GPU builder's entry points are never reached with the SAH builder; they are defined here only to satisfy the linker.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../stratum_amd/csrc/bvh_build.h"

namespace sthip {
bool lbvh_build_gpu(const std::vector<BvhTri>&, std::vector<BvhNode>&, std::vector<BvhTri>&, uint32_t&, uint32_t&, float&, std::string& err) {
  err = "no device in this program";
  return false;
}
bool lbvh_build_device(const DeviceBuildTarget&, const std::vector<MeshPiece>&, uint32_t, uint32_t, uint32_t&, uint32_t&, float*, float&, std::string& err, std::vector<FrontierEntry>*, uint32_t) {
  err = "no device in this program";
  return false;
}
}  // namespace sthip

template <typename T>
static std::vector<T> slurp(const std::string& path, bool must = true) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) {
    if (!must) return {};
    std::fprintf(stderr, "cannot open %s\n", path.c_str());
    std::exit(2);
  }
  const size_t n = (size_t)f.tellg();
  std::vector<T> v(n / sizeof(T));
  f.seekg(0);
  f.read((char*)v.data(), v.size() * sizeof(T));
  return v;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: top_level_ref <dir> <case>...\n");
    return 2;
  }
  const std::string d = argv[1];
  auto vertices = slurp<sthip_PackedVertexData>(d + "/vertices.bin");
  auto indices = slurp<uint8_t>(d + "/indices.bin");
  auto instances = slurp<sthip_InstanceData>(d + "/instances.bin");
  auto xf = slurp<sthip_TransformData>(d + "/xf.bin");
  auto inv = slurp<sthip_TransformData>(d + "/inv_xf.bin");
  auto materials = slurp<uint8_t>(d + "/materials.bin");
  std::vector<std::vector<uint8_t>> grids;
  for (int k = 0;; k++) {
    auto g = slurp<uint8_t>(d + "/volume" + std::to_string(k) + ".bin", false);
    if (g.empty()) break;
    grids.push_back(std::move(g));
  }
  std::vector<sthip_volume_desc> volumes;
  for (auto& g : grids) volumes.push_back(sthip_volume_desc{g.data(), (uint32_t)g.size()});
  indices.resize(indices.size() + 8, 0);
  sthip_scene_desc s{};
  s.gVertices = vertices.data();
  s.vertex_count = (uint32_t)vertices.size();
  s.gIndices = indices.data();
  s.indices_bytes = indices.size() - 8;
  s.gInstances = instances.data();
  s.gInstanceTransforms = xf.data();
  s.gInstanceInverseTransforms = inv.data();
  s.instance_count = (uint32_t)instances.size();
  s.gMaterialData = materials.data();
  s.material_bytes = materials.size();
  s.gVolumes = volumes.empty() ? nullptr : volumes.data();
  s.volume_count = (uint32_t)volumes.size();
  sthip::BuiltBvh built;
  std::string err;
  if (!sthip::build_scene_bvh(s, built, err, sthip::BVH_BUILDER_SAH_HOST, nullptr, false)) {
    std::printf("BUILD FAILED: %s\n", err.c_str());
    return 1;
  }
  for (int c = 2; c < argc; c++) {
    const std::string name = argv[c];
    auto nxf = slurp<sthip_TransformData>(d + "/" + name + "_xf.bin");
    auto ninv = slurp<sthip_TransformData>(d + "/" + name + "_inv.bin");
    if (nxf.size() != instances.size() || ninv.size() != instances.size()) {
      std::printf("%s: wrong matrix count\n", name.c_str());
      return 1;
    }
    sthip::TopLevelState st = built.top;
    std::vector<BvhNode> tlas;
    uint32_t root = 0, world = 1, depth = 0;
    float center[3] = {built.scene_center[0], built.scene_center[1], built.scene_center[2]}, radius = built.scene_radius;
    if (!sthip::rebuild_top_level(st, nxf.data(), ninv.data(), (uint32_t)instances.size(), tlas, root, world, depth, center, radius, err)) {
      std::printf("%s: REBUILD FAILED: %s\n", name.c_str(), err.c_str());
      return 1;
    }
    const uint32_t m = (uint32_t)st.entries.size();
    std::vector<float> boxes(6 * (size_t)m, 0.0f);
    std::vector<uint32_t> seen(m, 0);
    for (const BvhNode& nd : tlas)
      for (int k = 0; k < 2; k++) {
        const uint32_t r = nd.ref[k];
        if ((r & (BVH_LEAF_BIT | BVH_INST_BIT)) != (BVH_LEAF_BIT | BVH_INST_BIT) || r == BVH_INVALID_REF) continue;
        const uint32_t e = r & 0xFFFFu;
        if (e >= m) {
          std::printf("%s: entry out of range\n", name.c_str());
          return 1;
        }
        const float* xy = k == 0 ? nd.n0xy : nd.n1xy;
        float* b = &boxes[6 * (size_t)e];
        b[0] = xy[0], b[3] = xy[1], b[1] = xy[2], b[4] = xy[3], b[2] = nd.nz[2 * k], b[5] = nd.nz[2 * k + 1];
        seen[e]++;
      }
    if (tlas.empty() && m == 1) {  // the walk starts at the merged mesh: its kept box
      memcpy(boxes.data(), st.merged_box, 24);
      seen[0] = 1;
    }
    for (uint32_t e = 0; e < m; e++)
      if (!seen[e]) {
        std::printf("%s: entry %u is in no leaf\n", name.c_str(), e);
        return 1;
      }
    std::ofstream out(d + "/" + name + "_ref.bin", std::ios::binary);
    const uint32_t nodes = (uint32_t)tlas.size();
    out.write((const char*)&m, 4);
    out.write((const char*)boxes.data(), boxes.size() * sizeof(float));
    out.write((const char*)center, 12);
    out.write((const char*)&radius, 4);
    out.write((const char*)&nodes, 4);
    out.write((const char*)&world, 4);
    std::printf("%s: %u entries, %u nodes\n", name.c_str(), m, nodes);
  }
  return 0;
}
