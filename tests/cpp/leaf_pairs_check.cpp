// leaf_pairs_check.cpp — the leaf records of the 4-wide tree (stratum_amd/csrc/bvh.h: LeafPair; bvh_build.cpp:
// build_leaf_pairs) against the leaf triangles they stand for, as a plain CPU program (built with sanitizers by
// tests/test_leaf_pairs.py). Reads the raw scene arrays the test dumps:
//   leaf_pairs_check <dir>   with <dir>/{vertices,indices,instances,xf,inv_xf,materials}.bin
// For every triangle leaf the wide nodes refer to:
//   * there is a record at the index of its first triangle whose A = (p0, p1, p2) and whose B — (p0, p2, p3)
//     for LEAF_PAIR_FAN, (p1, p3, p2) for LEAF_PAIR_STRIP — are the vertices of BvhTri first and first + 1 bit for bit and in order,
//     with their ids; a LEAF_PAIR_SINGLE record belongs to a one-triangle leaf and carries an id of B that no triangle has;
//   * a LEAF_PAIR_SPLIT record belongs to a two-triangle leaf that fits neither pattern in either order — and every such leaf has
//     one — with A in it and B as a LEAF_PAIR_SINGLE record in the next slot; the wide nodes are left as they were;
//   * the triangles are the ones the build made before the records (as a multiset per leaf: the builder may swap the two).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../stratum_amd/csrc/bvh_build.h"

namespace sthip {
bool lbvh_build_gpu(const std::vector<BvhTri>&, std::vector<BvhNode>&, std::vector<BvhTri>&, uint32_t&, uint32_t&, float&, std::string& err) {
  err = "no device in this harness";
  return false;
}
bool lbvh_build_device(const DeviceBuildTarget&, const std::vector<MeshPiece>&, uint32_t, uint32_t, uint32_t&, uint32_t&, float*, float&, std::string& err, std::vector<FrontierEntry>*, uint32_t) {
  err = "no device in this harness";
  return false;
}
}  // namespace sthip

template <typename T>
static std::vector<T> slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path.c_str());
    std::exit(2);
  }
  const size_t n = (size_t)f.tellg();
  std::vector<T> v(n / sizeof(T));
  f.seekg(0);
  f.read((char*)v.data(), v.size() * sizeof(T));
  return v;
}

static bool same3(const float* a, const float* b) { return !memcmp(a, b, 12); }
static bool same_tri(const BvhTri& a, const BvhTri& b) { return !memcmp(&a, &b, sizeof(BvhTri)); }
// the patterns, stated once more: does (a, b) in this order fit one?
static bool fits(const BvhTri& a, const BvhTri& b) { return (same3(b.v0, a.v0) && same3(b.v1, a.v2)) || (same3(b.v0, a.v1) && same3(b.v2, a.v2)); }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string d = argv[1];
  auto vertices = slurp<sthip_PackedVertexData>(d + "/vertices.bin");
  auto indices = slurp<uint8_t>(d + "/indices.bin");
  auto instances = slurp<sthip_InstanceData>(d + "/instances.bin");
  auto xf = slurp<sthip_TransformData>(d + "/xf.bin");
  auto inv = slurp<sthip_TransformData>(d + "/inv_xf.bin");
  auto materials = slurp<uint8_t>(d + "/materials.bin");
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
  sthip::BuiltBvh b;
  std::string err;
  if (!sthip::build_scene_bvh(s, b, err)) return std::printf("BUILD FAILED: %s\n", err.c_str()), 1;
  sthip::build_wide_bvh(b);
  if (b.wide_nodes.empty()) return std::printf("FAIL: no wide nodes\n"), 1;
  const std::vector<BvhTri> before = b.tris;
  const std::vector<WideNode> wide_before = b.wide_nodes;
  sthip::build_leaf_pairs(b);
  if (b.leaf_pairs.size() != b.tris.size() || b.tris.size() != before.size()) return std::printf("FAIL: %zu records for %zu triangles\n", b.leaf_pairs.size(), b.tris.size()), 1;
  size_t single = 0, fan = 0, strip = 0, unfit = 0, swapped = 0;
  std::vector<uint8_t> seen(b.tris.size(), 0);
  for (size_t i = 0; i < b.wide_nodes.size(); i++) {
    const WideNode &w = b.wide_nodes[i], &w0 = wide_before[i];
    if (memcmp(&w, &w0, offsetof(WideNode, ref))) return std::printf("FAIL: build_leaf_pairs changed a wide node's boxes\n"), 1;
    for (int k = 0; k < 4; k++) {
      const uint32_t r = w.ref[k];
      const bool tri_leaf = (w0.ref[k] & (BVH_LEAF_BIT | BVH_INST_BIT)) == BVH_LEAF_BIT;
      if (r != w0.ref[k]) return std::printf("FAIL: build_leaf_pairs changed a reference\n"), 1;
      if (!tri_leaf || k >= (int)w.exp[3]) continue;
      const uint32_t first = (r & 0x3FFFFFFFu) >> 2, count = (r & 3u) + 1u;
      if (count > 2) return std::printf("FAIL: a leaf of %u triangles has records\n", count), 1;
      if (first + count > b.tris.size()) return std::printf("FAIL: leaf out of range\n"), 1;
      const bool again = seen[first] != 0;  // (a wrapped lone leaf fills two slots)
      seen[first] = 1;
      // the leaf's triangles are the build's, in either order
      const bool kept = same_tri(b.tris[first], before[first]) && (count == 1 || same_tri(b.tris[first + 1], before[first + 1]));
      const bool swap = count == 2 && same_tri(b.tris[first], before[first + 1]) && same_tri(b.tris[first + 1], before[first]);
      if (!kept && !swap) return std::printf("FAIL: leaf %u holds other triangles than before\n", first), 1;
      if (!again && !kept) swapped++;
      const BvhTri& A = b.tris[first];
      const LeafPair& p = b.leaf_pairs[first];
      if (p.first != first) return std::printf("FAIL: record %u names leaf %u\n", first, p.first), 1;
      if (!same3(p.p0, A.v0) || !same3(p.p1, A.v1) || !same3(p.p2, A.v2) || p.id_a != A.id) return std::printf("FAIL: record %u: A is not BvhTri %u\n", first, first), 1;
      if (p.form == LEAF_PAIR_SPLIT) {  // exactly the two-triangle leaves that fit neither pattern in either order: B as a single record in the next slot
        if (count != 2) return std::printf("FAIL: a split record on a one-triangle leaf\n"), 1;
        const BvhTri& B = b.tris[first + 1];
        if (fits(A, B) || fits(B, A)) return std::printf("FAIL: leaf %u fits a pattern but is split\n", first), 1;
        const LeafPair& q = b.leaf_pairs[first + 1];
        if (p.id_b != 0xFFFFFFFFu || q.id_b != 0xFFFFFFFFu || q.form != LEAF_PAIR_SINGLE || q.first != first + 1) return std::printf("FAIL: split leaf %u: the records' forms\n", first), 1;
        if (!same3(q.p0, B.v0) || !same3(q.p1, B.v1) || !same3(q.p2, B.v2) || q.id_a != B.id) return std::printf("FAIL: split leaf %u: the second record is not BvhTri %u\n", first, first + 1), 1;
        if (!again) unfit++;
        continue;
      }
      if (p.form == LEAF_PAIR_SINGLE) {
        if (count != 1) return std::printf("FAIL: a single record on a two-triangle leaf\n"), 1;
        if (p.id_b != 0xFFFFFFFFu) return std::printf("FAIL: a single record exposes an id of B\n"), 1;
        for (const BvhTri& t : b.tris)
          if (t.id == p.id_b) return std::printf("FAIL: the id of a single record's B belongs to a triangle\n"), 1;
        if (!again) single++;
        continue;
      }
      if (count != 2) return std::printf("FAIL: a pair record on a one-triangle leaf\n"), 1;
      const BvhTri& B = b.tris[first + 1];
      if (!fits(A, B)) return std::printf("FAIL: leaf %u has a pair record but fits no pattern\n", first), 1;
      const float *b0, *b1, *b2;
      if (p.form == LEAF_PAIR_FAN) b0 = p.p0, b1 = p.p2, b2 = p.p3;
      else if (p.form == LEAF_PAIR_STRIP) b0 = p.p1, b1 = p.p3, b2 = p.p2;
      else return std::printf("FAIL: record %u has form %u\n", first, p.form), 1;
      if (!same3(b0, B.v0) || !same3(b1, B.v1) || !same3(b2, B.v2) || p.id_b != B.id) return std::printf("FAIL: record %u: B is not BvhTri %u\n", first, first + 1), 1;
      if (!again) (p.form == LEAF_PAIR_FAN ? fan : strip)++;
    }
  }
  if (single != b.pair_single || fan != b.pair_fan || strip != b.pair_strip || unfit != b.pair_unfit || swapped != b.pair_swapped)
    return std::printf("FAIL: the builder counted %zu / %zu / %zu / %zu (%zu swapped), the check %zu / %zu / %zu / %zu (%zu)\n", b.pair_single, b.pair_fan, b.pair_strip, b.pair_unfit, b.pair_swapped, single, fan,
                       strip, unfit, swapped), 1;
  // embedded leaves take no records
  {
    sthip::BuiltBvh e;
    if (!sthip::build_scene_bvh(s, e, err, sthip::BVH_BUILDER_SAH_HOST, nullptr, true)) return std::printf("BUILD FAILED: %s\n", err.c_str()), 1;
    sthip::build_wide_bvh(e);
    const std::vector<WideNode> w0 = e.wide_nodes;
    sthip::build_leaf_pairs(e);
    if (!e.leaf_pairs.empty() || (!w0.empty() && memcmp(w0.data(), e.wide_nodes.data(), w0.size() * sizeof(WideNode)))) return std::printf("FAIL: records for embedded leaves\n"), 1;
  }
  std::printf("LEAF PAIRS OK single %zu fan %zu strip %zu unfit %zu swapped %zu of %zu triangles\n", single, fan, strip, unfit, swapped, b.tris.size());
  return 0;
}
