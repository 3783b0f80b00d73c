// first_hit_key_check.cpp — csrc/first_hits.h on the host (no HIP): equal inputs give equal keys, every field of the key
// changes equality when it alone changes, and making a key reads exactly view_count records of the view arrays (they are
// heap blocks of exactly that size here: built with -fsanitize=address,undefined a read past them ends the program).
#include <stdio.h>

#include <vector>

#include "../../stratum_amd/csrc/first_hits.h"

using namespace sthip;

namespace {
int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    printf("FAIL: %s\n", what);
    failures++;
  }
}

struct Inputs {
  uint64_t serial = 7;
  uint32_t extent[2] = {128, 64};
  uint32_t view_count = 2;
  uint32_t max_path_vertices = 4;
  uint32_t shard_rank = 0, shard_count = 2, tile_w = 64, tile_h = 32;
  uint32_t paths_per_seed = 2048;
  bool alpha_test = false, flip_uvs = false;
  sthip_ViewData* views = nullptr;  // exactly view_count records each
  sthip_TransformData* xf = nullptr;
  explicit Inputs(uint32_t n = 2) : view_count(n) {
    views = new sthip_ViewData[n];
    xf = new sthip_TransformData[n];
    for (uint32_t v = 0; v < n; v++) {
      sthip_ViewData& w = views[v];
      w.projection.scale[0] = 1.5f + (float)v;
      w.projection.scale[1] = 2.5f;
      w.projection.offset[0] = 0.0f;
      w.projection.offset[1] = 0.25f;
      w.projection.near_plane = -0.01f;
      w.projection.far_plane = 100.0f;
      w.projection.sensor_area = 1.0f;
      w.projection.vertical_fov = 0.7f;
      w.image_min[0] = (int32_t)(v * 64);
      w.image_min[1] = 0;
      w.image_max[0] = (int32_t)(v * 64 + 64);
      w.image_max[1] = 64;
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) xf[v].m[r][c] = r == c ? 1.0f : (c == 3 ? (float)(v + r) : 0.0f);
    }
  }
  Inputs(const Inputs&) = delete;
  Inputs& operator=(const Inputs&) = delete;
  ~Inputs() {
    delete[] views;
    delete[] xf;
  }
  bool make(FirstHitKey& k) const {
    return first_hit_key_make(k, serial, extent, view_count, max_path_vertices, shard_rank, shard_count, tile_w, tile_h, paths_per_seed, alpha_test, flip_uvs, views, xf);
  }
};

// `change` alters one input of a fresh set: the key must then differ from the unchanged set's, in both argument orders
template <typename F>
void differs(const char* what, F&& change) {
  Inputs a, b;
  change(b);
  FirstHitKey ka, kb;
  expect(a.make(ka) && b.make(kb), what);
  expect(!first_hit_key_equal(ka, kb) && !first_hit_key_equal(kb, ka), what);
}
}  // namespace

int main() {
  {  // equal inputs, separately allocated: equal keys; a key equals itself
    Inputs a, b;
    FirstHitKey ka, kb;
    expect(a.make(ka) && b.make(kb), "equal inputs make keys");
    expect(first_hit_key_equal(ka, kb) && first_hit_key_equal(kb, ka) && first_hit_key_equal(ka, ka), "equal inputs compare equal");
  }
  {  // a key that was never made, or could not be made, equals nothing
    FirstHitKey never;
    memset(&never, 0, sizeof never);
    expect(!first_hit_key_equal(never, never), "an unmade key equals nothing");
    Inputs a;
    FirstHitKey k;
    expect(!first_hit_key_make(k, 1, a.extent, 0, 4, 0, 1, 64, 32, 2048, false, false, a.views, a.xf) && !first_hit_key_equal(k, k), "no views: no key");
    expect(!first_hit_key_make(k, 1, a.extent, FIRST_HITS_MAX_VIEWS + 1, 4, 0, 1, 64, 32, 2048, false, false, a.views, a.xf) && !first_hit_key_equal(k, k), "too many views: no key (and nothing read)");
    expect(!first_hit_key_make(k, 1, a.extent, 2, 4, 0, 1, 64, 32, 2048, false, false, nullptr, a.xf) && !first_hit_key_make(k, 1, a.extent, 2, 4, 0, 1, 64, 32, 2048, false, false, a.views, nullptr),
           "a missing array: no key");
  }
  differs("scene serial", [](Inputs& b) { b.serial++; });
  differs("extent x", [](Inputs& b) { b.extent[0] = 64; });
  differs("extent y", [](Inputs& b) { b.extent[1] = 128; });
  differs("extent swapped (same pixel count)", [](Inputs& b) { b.extent[0] = 64, b.extent[1] = 128; });
  differs("gMaxPathVertices 4 -> 1", [](Inputs& b) { b.max_path_vertices = 1; });
  differs("shard rank", [](Inputs& b) { b.shard_rank = 1; });
  differs("shard count", [](Inputs& b) { b.shard_count = 3; });
  differs("tile width", [](Inputs& b) { b.tile_w = 32; });
  differs("tile height", [](Inputs& b) { b.tile_h = 16; });
  differs("paths per seed", [](Inputs& b) { b.paths_per_seed = 4096; });
  differs("alpha test", [](Inputs& b) { b.alpha_test = true; });
  differs("uv flip", [](Inputs& b) { b.flip_uvs = true; });
  {  // gMaxPathVertices only enters as "at least 2"
    Inputs a, b;
    b.max_path_vertices = 9;
    FirstHitKey ka, kb;
    expect(a.make(ka) && b.make(kb) && first_hit_key_equal(ka, kb), "gMaxPathVertices 4 and 9 share a key");
  }
  // every 32-bit word of every view record and of every view transform, one at a time
  for (uint32_t v = 0; v < 2; v++) {
    for (size_t w = 0; w < sizeof(sthip_ViewData) / 4; w++)
      differs("a word of a view", [&](Inputs& b) { reinterpret_cast<uint32_t*>(&b.views[v])[w] ^= 0x00400000u; });
    for (size_t w = 0; w < sizeof(sthip_TransformData) / 4; w++)
      differs("a word of a view transform", [&](Inputs& b) { reinterpret_cast<uint32_t*>(&b.xf[v])[w] ^= 0x00400000u; });
  }
  {  // the view count alone: the first view of two against that view alone
    Inputs two(2), one(1);
    memcpy(one.views, two.views, sizeof(sthip_ViewData));
    memcpy(one.xf, two.xf, sizeof(sthip_TransformData));
    FirstHitKey k2, k1;
    expect(two.make(k2) && one.make(k1) && !first_hit_key_equal(k2, k1) && !first_hit_key_equal(k1, k2), "view count");
  }
  // view counts 1 .. the maximum: arrays of exactly that many records are enough; what lies behind them in the key is zero
  for (uint32_t n = 1; n <= FIRST_HITS_MAX_VIEWS; n++) {
    Inputs a(n), b(n);
    FirstHitKey ka, kb;
    expect(a.make(ka) && b.make(kb) && first_hit_key_equal(ka, kb), "n views make equal keys");
    std::vector<unsigned char> zero(sizeof(sthip_ViewData) + sizeof(sthip_TransformData), 0);
    for (uint32_t v = n; v < FIRST_HITS_MAX_VIEWS; v++)
      expect(!memcmp(&ka.views[v], zero.data(), sizeof(sthip_ViewData)) && !memcmp(&ka.view_xf[v], zero.data(), sizeof(sthip_TransformData)), "records behind view_count are zero");
    reinterpret_cast<uint32_t*>(&b.xf[n - 1])[11] ^= 1u;  // the last word of the last record is part of the key
    expect(b.make(kb) && !first_hit_key_equal(ka, kb), "the last record counts");
  }
  if (failures) return 1;
  printf("FIRST HIT KEY OK\n");
  return 0;
}
