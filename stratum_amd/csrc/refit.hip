// refit.hip — deforming meshes: the leaf triangles are gathered again from gVertices and the boxes of the bottom levels are
// refitted bottom-up, all on the device and in place (sthip_scene_update_vertices, api.hip). Topology stays: the same index
// buffer, the same trees, the same leaf order.
//
// The reference rebuilds a mesh's BLAS whenever the mesh is dirty (src/Node/Scene.cpp:345,435-459). Closest hit is the
// minimum over all triangles with ties broken by id, so a frame does not depend on the shape of the tree: a refitted tree
// gives the frame a fresh build gives, and costs one pass over triangles and nodes instead of a sort and a build.
//
// Gather: one lane per leaf triangle reads its index triple and its three vertices through BvhTri::src_indices / src_vertex
// and rewrites the three positions (bit copies; id and the src words stay).
//
// Refit: level-synchronous. A schedule — the bottom-level nodes that can be reached from the entries' roots, grouped by
// height — is made once per resident tree (the GPU builder leaves dead nodes in the array, where its host-built SAH top
// replaced PLOC's: only reachability says which nodes are the tree) and kept until the next upload. A refit is then one
// launch per height: a node reads its leaf children's triangles or its inner children's exact boxes (written by an EARLIER
// launch: the kernel boundary is the release / acquire, the L2s of the XCDs are not coherent with each other inside a
// launch) from a scratch array of exact binary32 boxes, writes its own exact box there, and packs its child boxes with
// pack_plane (bvh_build.h), the outward rounding of every upload. The packed planes are never read back as boxes, so
// two refits over the same vertices give the same bytes and the rounding does not compound. The scratch record also
// carries the SAH cost of the node's subtree, so the pass ends with every root's box and cost: one small read-back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "bvh_build.h"

namespace sthip {

struct DeviceRefit {
  // schedule (valid: made for the tree that is resident)
  bool valid = false;
  uint32_t blas_nodes = 0;
  uint32_t scheduled = 0;               // nodes in the schedule
  std::vector<uint32_t> height_begin;   // [h] .. [h + 1]: the nodes of height h + 1 in `sched`
  std::vector<uint32_t> roots;          // distinct bottom-level roots, in the order of their first entry
  double sah_at_build = 0;
  uint32_t* sched = nullptr;   // node indices grouped by height
  uint32_t* list = nullptr;    // the same nodes grouped by depth (schedule construction)
  uint32_t* mark = nullptr;
  uint32_t* height = nullptr;
  uint32_t* counts = nullptr;  // [0, levels]: nodes per depth; [levels + 1, 2 levels + 1]: per height; then cursors per height; last: failure flag
  uint32_t* offsets = nullptr;  // exclusive scan of the per-height counts
  float4* box = nullptr;       // 2 per node: (lo.xyz, SAH cost of the subtree), (hi.xyz, 0)
  uint32_t* roots_dev = nullptr;
  float4* out_dev = nullptr;   // 2 per root, then 2 per emitter
  uint32_t* readback = nullptr;  // pinned
  size_t node_capacity = 0, level_capacity = 0, root_capacity = 0, readback_words = 0;
  hipEvent_t ev[2] = {nullptr, nullptr};
};

DeviceRefit* device_refit_create() { return new DeviceRefit(); }
void device_refit_invalidate(DeviceRefit* s) {
  if (s) s->valid = false;
}
void device_refit_destroy(DeviceRefit* s) {
  if (!s) return;
  (void)hipFree(s->sched);
  (void)hipFree(s->list);
  (void)hipFree(s->mark);
  (void)hipFree(s->height);
  (void)hipFree(s->counts);
  (void)hipFree(s->offsets);
  (void)hipFree(s->box);
  (void)hipFree(s->roots_dev);
  (void)hipFree(s->out_dev);
  if (s->readback) (void)hipHostFree(s->readback);
  for (int k = 0; k < 2; k++)
    if (s->ev[k]) (void)hipEventDestroy(s->ev[k]);
  delete s;
}

namespace {

constexpr unsigned REFIT_BLOCK = 256;

// tests: STHIP_POISON_ALLOC=<byte> (context.h, DevBuf::ensure) fills every new buffer of the refit too, the pinned read-back
// staging included, so that a read of a record no launch has written shows in a fresh process, where new memory is zero pages
int poison_byte() {
  static const int poison = [] {
    const char* v = getenv("STHIP_POISON_ALLOC");
    return v && *v ? (int)(strtoul(v, nullptr, 0) & 0xFFu) : -1;
  }();
  return poison;
}
template <typename T>
hipError_t refit_malloc(T** p, size_t bytes) {
  hipError_t e = hipMalloc((void**)p, bytes);
  if (e == hipSuccess && poison_byte() >= 0) e = hipMemset(*p, poison_byte(), bytes);
  return e;
}
hipError_t refit_host_malloc(uint32_t** p, size_t bytes) {
  const hipError_t e = hipHostMalloc((void**)p, bytes);
  if (e == hipSuccess && poison_byte() >= 0) memset(*p, poison_byte(), bytes);
  return e;
}

__device__ inline uint32_t as_u32(float f) { return __float_as_uint(f); }
// the child references of a packed node: the low mantissa bytes of its eight x / y planes (bvh.h)
__device__ inline void node_refs(const float4& a, const float4& b, uint32_t& r0, uint32_t& r1) {
  r0 = (as_u32(a.x) & 0xFFu) | ((as_u32(a.y) & 0xFFu) << 8) | ((as_u32(a.z) & 0xFFu) << 16) | ((as_u32(a.w) & 0xFFu) << 24);
  r1 = (as_u32(b.x) & 0xFFu) | ((as_u32(b.y) & 0xFFu) << 8) | ((as_u32(b.z) & 0xFFu) << 16) | ((as_u32(b.w) & 0xFFu) << 24);
}
__device__ inline bool is_inner(uint32_t r) { return !(r & BVH_LEAF_BIT); }
__device__ inline bool is_tri_leaf(uint32_t r) { return (r & BVH_LEAF_BIT) && !(r & BVH_INST_BIT); }

// ---- gather ----
__global__ void __launch_bounds__(REFIT_BLOCK) k_refit_gather(float4* tris, uint32_t tri_count, const float4* vertices, uint32_t vertex_count, const uint8_t* indices, uint64_t indices_bytes) {
  for (uint32_t i = blockIdx.x * REFIT_BLOCK + threadIdx.x; i < tri_count; i += gridDim.x * REFIT_BLOCK) {
    float4 t0 = tris[3 * (size_t)i], t1 = tris[3 * (size_t)i + 1], t2 = tris[3 * (size_t)i + 2];
    const uint32_t src_indices = as_u32(t1.w), src_vertex = as_u32(t2.w);
    const uint32_t stride = (src_vertex >> 31) ? 4u : 2u, first = src_vertex & 0x7FFFFFFFu;
    if ((uint64_t)src_indices + 3u * stride > indices_bytes) continue;  // (the builders have refused such scenes already)
    uint32_t idx[3];
    bool ok = true;
    for (int k = 0; k < 3; k++) {  // byte loads: an index buffer's byte offset need not be aligned to its stride
      const uint8_t* q = indices + (size_t)src_indices + (size_t)k * stride;
      idx[k] = stride == 2u ? ((uint32_t)q[0] | (uint32_t)q[1] << 8) : ((uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24);
      idx[k] += first;
      ok = ok && idx[k] < vertex_count;
    }
    if (!ok) continue;
    const float4 a = vertices[2 * (size_t)idx[0]], b = vertices[2 * (size_t)idx[1]], c = vertices[2 * (size_t)idx[2]];  // position.xyz | u
    t0.x = a.x, t0.y = a.y, t0.z = a.z;
    t1.x = b.x, t1.y = b.y, t1.z = b.z;
    t2.x = c.x, t2.y = c.y, t2.z = c.z;
    tris[3 * (size_t)i] = t0;
    tris[3 * (size_t)i + 1] = t1;
    tris[3 * (size_t)i + 2] = t2;
  }
}

// ---- schedule ----
__global__ void k_sched_seed(const uint32_t* roots, uint32_t root_count, uint32_t node_count, uint32_t* mark, uint32_t* list, uint32_t* counts, uint32_t* fail) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint32_t n = 0;
  for (uint32_t r = 0; r < root_count; r++) {
    if (roots[r] >= node_count) {
      *fail = 2u;
      continue;
    }
    mark[roots[r]] = 1u;
    list[n++] = roots[r];
  }
  counts[0] = n;
}
// the first item of depth `level` in the list, and how many there are
__device__ inline void level_range(const uint32_t* counts, uint32_t level, uint32_t& base, uint32_t& n) {
  __shared__ uint32_t s_base;
  if (threadIdx.x == 0) {
    uint32_t b = 0;
    for (uint32_t l = 0; l < level; l++) b += counts[l];
    s_base = b;
  }
  __syncthreads();
  base = s_base;
  n = counts[level];
}
// top down: the children of depth `level` become depth `level + 1` (counts[level + 1] is only added to by this launch)
__global__ void __launch_bounds__(REFIT_BLOCK) k_sched_down(const BvhNodeSlot* nodes, uint32_t node_count, uint32_t* list, uint32_t* counts, uint32_t level, uint32_t* mark, uint32_t* fail) {
  uint32_t base, n;
  level_range(counts, level, base, n);
  const float4* words = reinterpret_cast<const float4*>(nodes);
  constexpr size_t W = sizeof(BvhNodeSlot) / 16;
  for (uint32_t item = blockIdx.x * REFIT_BLOCK + threadIdx.x; item < n; item += gridDim.x * REFIT_BLOCK) {
    const uint32_t i = list[base + item];
    uint32_t r[2];
    node_refs(words[W * i], words[W * i + 1], r[0], r[1]);
    for (int c = 0; c < 2; c++) {
      if (!is_inner(r[c])) continue;
      if (r[c] >= node_count) {
        atomicOr(fail, 2u);
        continue;
      }
      if (atomicExch(&mark[r[c]], 1u) != 0u) continue;
      const uint32_t at = base + n + atomicAdd(&counts[level + 1], 1u);
      if (at < node_count) list[at] = r[c];
    }
  }
}
// bottom up over the depths: height = 1 + the largest height among the inner children (0: only leaves below)
__global__ void __launch_bounds__(REFIT_BLOCK) k_sched_height(const BvhNodeSlot* nodes, uint32_t node_count, const uint32_t* list, const uint32_t* counts, uint32_t level, uint32_t* height, uint32_t* hcounts,
                                                              uint32_t max_height) {
  uint32_t base, n;
  level_range(counts, level, base, n);
  const float4* words = reinterpret_cast<const float4*>(nodes);
  constexpr size_t W = sizeof(BvhNodeSlot) / 16;
  for (uint32_t item = blockIdx.x * REFIT_BLOCK + threadIdx.x; item < n; item += gridDim.x * REFIT_BLOCK) {
    const uint32_t i = list[base + item];
    uint32_t r[2], h = 0;
    node_refs(words[W * i], words[W * i + 1], r[0], r[1]);
    for (int c = 0; c < 2; c++)
      if (is_inner(r[c]) && r[c] < node_count) h = max(h, height[r[c]] + 1u);
    h = min(h, max_height);
    height[i] = h;
    atomicAdd(&hcounts[h], 1u);
  }
}
__global__ void __launch_bounds__(REFIT_BLOCK) k_sched_scatter(const uint32_t* list, uint32_t n, const uint32_t* height, const uint32_t* offsets, uint32_t* cursors, uint32_t* sched) {
  for (uint32_t k = blockIdx.x * REFIT_BLOCK + threadIdx.x; k < n; k += gridDim.x * REFIT_BLOCK) {
    const uint32_t i = list[k], h = height[i];
    sched[offsets[h] + atomicAdd(&cursors[h], 1u)] = i;  // (the order inside a height does not matter: every node writes only its own records)
  }
}

// ---- refit ----
struct Box3 {
  float lo[3], hi[3];
};
__device__ inline float box_area(const Box3& b) {
  const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
  if (!(dx >= 0 && dy >= 0 && dz >= 0)) return 0.0f;  // inverted (empty) box
  return dx * dy + dy * dz + dz * dx;
}
__device__ inline void grow(Box3& b, const float4& p) {
  b.lo[0] = fminf(b.lo[0], p.x), b.lo[1] = fminf(b.lo[1], p.y), b.lo[2] = fminf(b.lo[2], p.z);
  b.hi[0] = fmaxf(b.hi[0], p.x), b.hi[1] = fmaxf(b.hi[1], p.y), b.hi[2] = fmaxf(b.hi[2], p.z);
}
// One node of the height this launch serves. WRITE = false: the boxes and costs of the tree as it is (the cost at build).
template <bool WRITE>
__global__ void __launch_bounds__(REFIT_BLOCK) k_refit_level(BvhNodeSlot* nodes, uint32_t node_count, const uint32_t* sched, uint32_t begin, uint32_t count, const float4* tris, uint32_t tri_count, float4* box) {
  float4* words = reinterpret_cast<float4*>(nodes);
  constexpr size_t W = sizeof(BvhNodeSlot) / 16;
  for (uint32_t item = blockIdx.x * REFIT_BLOCK + threadIdx.x; item < count; item += gridDim.x * REFIT_BLOCK) {
    const uint32_t i = sched[begin + item];
    if (i >= node_count) continue;
    const float4 w0 = words[W * i], w1 = words[W * i + 1], w2 = words[W * i + 2];
    uint32_t r[2];
    node_refs(w0, w1, r[0], r[1]);
    Box3 cb[2], own;
    bool have[2] = {false, false};
    float cost = 0.0f;
    const float inf = __builtin_inff();
    for (int a = 0; a < 3; a++) own.lo[a] = inf, own.hi[a] = -inf;
    for (int c = 0; c < 2; c++) {
      Box3& b = cb[c];
      for (int a = 0; a < 3; a++) b.lo[a] = inf, b.hi[a] = -inf;
      if (is_inner(r[c])) {
        if (r[c] >= node_count) continue;
        const float4 lo = box[2 * (size_t)r[c]], hi = box[2 * (size_t)r[c] + 1];
        b.lo[0] = lo.x, b.lo[1] = lo.y, b.lo[2] = lo.z;
        b.hi[0] = hi.x, b.hi[1] = hi.y, b.hi[2] = hi.z;
        cost += lo.w;
        have[c] = true;
      } else if (is_tri_leaf(r[c])) {
        const uint32_t first = (r[c] & 0x3FFFFFFFu) >> 2, n = (r[c] & 3u) + 1u;
        if ((uint64_t)first + n > tri_count) continue;
        for (uint32_t k = 0; k < n; k++) {
          grow(b, tris[3 * (size_t)(first + k)]);
          grow(b, tris[3 * (size_t)(first + k) + 1]);
          grow(b, tris[3 * (size_t)(first + k) + 2]);
        }
        cost += box_area(b) * (float)n;
        have[c] = true;
      }  // (an empty child keeps the planes it has)
      if (have[c])
        for (int a = 0; a < 3; a++) own.lo[a] = fminf(own.lo[a], b.lo[a]), own.hi[a] = fmaxf(own.hi[a], b.hi[a]);
    }
    cost += box_area(own);
    box[2 * (size_t)i] = make_float4(own.lo[0], own.lo[1], own.lo[2], cost);
    box[2 * (size_t)i + 1] = make_float4(own.hi[0], own.hi[1], own.hi[2], 0.0f);
    if (WRITE) {
      float4 o0 = w0, o1 = w1, o2 = w2;
      if (have[0]) {
        o0.x = __uint_as_float(pack_plane(cb[0].lo[0], false, r[0]));
        o0.y = __uint_as_float(pack_plane(cb[0].hi[0], true, r[0] >> 8));
        o0.z = __uint_as_float(pack_plane(cb[0].lo[1], false, r[0] >> 16));
        o0.w = __uint_as_float(pack_plane(cb[0].hi[1], true, r[0] >> 24));
        o2.x = cb[0].lo[2];
        o2.y = cb[0].hi[2];
      }
      if (have[1]) {
        o1.x = __uint_as_float(pack_plane(cb[1].lo[0], false, r[1]));
        o1.y = __uint_as_float(pack_plane(cb[1].hi[0], true, r[1] >> 8));
        o1.z = __uint_as_float(pack_plane(cb[1].lo[1], false, r[1] >> 16));
        o1.w = __uint_as_float(pack_plane(cb[1].hi[1], true, r[1] >> 24));
        o2.z = cb[1].lo[2];
        o2.w = cb[1].hi[2];
      }
      words[W * i] = o0;
      words[W * i + 1] = o1;
      words[W * i + 2] = o2;
    }
  }
}
__global__ void k_refit_roots(const float4* box, const uint32_t* roots, uint32_t root_count, float4* out) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= root_count) return;
  out[2 * r] = box[2 * (size_t)roots[r]];
  out[2 * r + 1] = box[2 * (size_t)roots[r] + 1];
}
// The box of the vertices an emissive instance's triangles refer to (bvh.h: EmitterBounds before its padding): one block
// per instance, minima and maxima are exact whatever the order.
__global__ void __launch_bounds__(REFIT_BLOCK) k_refit_emitter_boxes(const sthip_InstanceData* instances, const uint32_t* emitter_instance, const float4* vertices, uint32_t vertex_count, const uint8_t* indices,
                                                                     uint64_t indices_bytes, float4* out) {
  __shared__ float s_lo[3][REFIT_BLOCK], s_hi[3][REFIT_BLOCK];
  const sthip_InstanceData in = instances[emitter_instance[blockIdx.x]];
  const uint32_t prims = (in.packed[1] >> 12) & 0xFFFFu, stride = in.packed[1] >> 28, first_vertex = in.packed[2];
  const uint64_t at = in.packed[3];
  const float inf = __builtin_inff();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  for (uint32_t k = threadIdx.x; k < 3 * prims; k += REFIT_BLOCK) {
    const uint64_t byte = at + (uint64_t)k * (stride == 2u ? 2u : 4u);
    if (byte + (stride == 2u ? 2u : 4u) > indices_bytes) continue;
    const uint8_t* q = indices + byte;
    const uint32_t index = stride == 2u ? ((uint32_t)q[0] | (uint32_t)q[1] << 8) : ((uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24);
    if ((uint64_t)first_vertex + index >= vertex_count) continue;
    const float4 p = vertices[2 * (size_t)(first_vertex + index)];
    lo[0] = fminf(lo[0], p.x), lo[1] = fminf(lo[1], p.y), lo[2] = fminf(lo[2], p.z);
    hi[0] = fmaxf(hi[0], p.x), hi[1] = fmaxf(hi[1], p.y), hi[2] = fmaxf(hi[2], p.z);
  }
  for (int a = 0; a < 3; a++) s_lo[a][threadIdx.x] = lo[a], s_hi[a][threadIdx.x] = hi[a];
  __syncthreads();
  for (unsigned step = REFIT_BLOCK / 2; step > 0; step >>= 1) {
    if (threadIdx.x < step)
      for (int a = 0; a < 3; a++) {
        s_lo[a][threadIdx.x] = fminf(s_lo[a][threadIdx.x], s_lo[a][threadIdx.x + step]);
        s_hi[a][threadIdx.x] = fmaxf(s_hi[a][threadIdx.x], s_hi[a][threadIdx.x + step]);
      }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[2 * blockIdx.x] = make_float4(s_lo[0][0], s_lo[1][0], s_lo[2][0], 0.0f);
    out[2 * blockIdx.x + 1] = make_float4(s_hi[0][0], s_hi[1][0], s_hi[2][0], 0.0f);
  }
}

inline unsigned grid_of(size_t n) { return (unsigned)std::max<size_t>(1, std::min<size_t>(8192, (n + REFIT_BLOCK - 1) / REFIT_BLOCK)); }

}  // namespace

#define REFIT_TRY(x)                                        \
  do {                                                      \
    const hipError_t e_ = (x);                              \
    if (e_ != hipSuccess) {                                 \
      err = std::string(#x) + ": " + hipGetErrorString(e_); \
      return false;                                         \
    }                                                       \
  } while (0)

namespace {
// the per-height launches over the schedule, then the roots' records to out_dev
void launch_refit(DeviceRefit* s, bool write, BvhNodeSlot* nodes, const BvhTri* tris, uint32_t tri_count, hipStream_t st) {
  for (size_t h = 0; h + 1 < s->height_begin.size(); h++) {
    const uint32_t begin = s->height_begin[h], count = s->height_begin[h + 1] - begin;
    if (!count) continue;
    if (write)
      hipLaunchKernelGGL(k_refit_level<true>, dim3(grid_of(count)), dim3(REFIT_BLOCK), 0, st, nodes, s->blas_nodes, s->sched, begin, count, reinterpret_cast<const float4*>(tris), tri_count, s->box);
    else
      hipLaunchKernelGGL(k_refit_level<false>, dim3(grid_of(count)), dim3(REFIT_BLOCK), 0, st, nodes, s->blas_nodes, s->sched, begin, count, reinterpret_cast<const float4*>(tris), tri_count, s->box);
  }
  const uint32_t roots = (uint32_t)s->roots.size();
  if (roots) hipLaunchKernelGGL(k_refit_roots, dim3((roots + 63) / 64), dim3(64), 0, st, s->box, s->roots_dev, roots, s->out_dev);
}
// sum of the roots' subtree costs over the sum of the roots' areas, in the order of the roots
double sah_of(const float* rec, size_t roots) {
  double cost = 0, area = 0;
  for (size_t r = 0; r < roots; r++) {
    const float* lo = rec + 8 * r;
    const float* hi = lo + 4;
    const double dx = (double)hi[0] - lo[0], dy = (double)hi[1] - lo[1], dz = (double)hi[2] - lo[2];
    if (!(dx >= 0 && dy >= 0 && dz >= 0)) continue;
    cost += lo[3];
    area += dx * dy + dy * dz + dz * dx;
  }
  return area > 0 ? cost / area : 0.0;
}
}  // namespace

bool refit_prepare(DeviceRefit* s, BvhNodeSlot* nodes, uint32_t blas_nodes, const std::vector<uint32_t>& roots, uint32_t max_levels, const BvhTri* tris, uint32_t tri_count, uint32_t max_emitters,
                   void* stream_, std::string& err) {
  hipStream_t st = (hipStream_t)stream_;
  if (!s) {
    err = "refit: no state";
    return false;
  }
  if (s->valid && s->blas_nodes == blas_nodes && s->roots == roots) return true;
  s->valid = false;
  const uint32_t levels = std::max(max_levels, 2u) + 8u;  // depths 0 .. levels - 1 may hold nodes; [levels] must stay empty
  if (blas_nodes > s->node_capacity) {
    (void)hipFree(s->sched);
    (void)hipFree(s->list);
    (void)hipFree(s->mark);
    (void)hipFree(s->height);
    (void)hipFree(s->box);
    s->sched = s->list = s->mark = s->height = nullptr;
    s->box = nullptr;
    s->node_capacity = 0;
    REFIT_TRY(refit_malloc(&s->sched, (size_t)blas_nodes * 4));
    REFIT_TRY(refit_malloc(&s->list, (size_t)blas_nodes * 4));
    REFIT_TRY(refit_malloc(&s->mark, (size_t)blas_nodes * 4));
    REFIT_TRY(refit_malloc(&s->height, (size_t)blas_nodes * 4));
    REFIT_TRY(refit_malloc(&s->box, (size_t)blas_nodes * 2 * sizeof(float4)));
    s->node_capacity = blas_nodes;
  }
  const size_t count_words = 3 * (size_t)(levels + 1) + 1;
  if (levels + 1 > s->level_capacity) {
    (void)hipFree(s->counts);
    (void)hipFree(s->offsets);
    s->counts = s->offsets = nullptr;
    s->level_capacity = 0;
    REFIT_TRY(refit_malloc(&s->counts, count_words * 4));
    REFIT_TRY(refit_malloc(&s->offsets, (size_t)(levels + 1) * 4));
    s->level_capacity = levels + 1;
  }
  const size_t out_records = roots.size() + max_emitters + 1;
  if (out_records > s->root_capacity) {
    (void)hipFree(s->roots_dev);
    (void)hipFree(s->out_dev);
    s->roots_dev = nullptr;
    s->out_dev = nullptr;
    s->root_capacity = 0;
    REFIT_TRY(refit_malloc(&s->roots_dev, out_records * 4));
    REFIT_TRY(refit_malloc(&s->out_dev, out_records * 2 * sizeof(float4)));
    s->root_capacity = out_records;
  }
  const size_t readback_words = std::max(count_words, out_records * 8);
  if (readback_words > s->readback_words) {
    if (s->readback) (void)hipHostFree(s->readback);
    s->readback = nullptr;
    s->readback_words = 0;
    REFIT_TRY(refit_host_malloc(&s->readback, readback_words * 4));
    s->readback_words = readback_words;
  }
  for (int k = 0; k < 2; k++)
    if (!s->ev[k]) REFIT_TRY(hipEventCreate(&s->ev[k]));
  s->blas_nodes = blas_nodes;
  s->roots = roots;
  s->height_begin.assign(1, 0u);
  s->scheduled = 0;
  s->sah_at_build = 0;
  if (roots.empty() || blas_nodes == 0) {  // (spheres and volumes only: nothing to refit)
    s->valid = true;
    return true;
  }
  uint32_t* depth_counts = s->counts;
  uint32_t* height_counts = s->counts + (levels + 1);
  uint32_t* cursors = s->counts + 2 * (size_t)(levels + 1);
  uint32_t* fail = s->counts + 3 * (size_t)(levels + 1);
  REFIT_TRY(hipMemcpyAsync(s->roots_dev, roots.data(), roots.size() * 4, hipMemcpyHostToDevice, st));
  REFIT_TRY(hipMemsetAsync(s->mark, 0, (size_t)blas_nodes * 4, st));
  REFIT_TRY(hipMemsetAsync(s->counts, 0, count_words * 4, st));
  hipLaunchKernelGGL(k_sched_seed, dim3(1), dim3(1), 0, st, s->roots_dev, (uint32_t)roots.size(), blas_nodes, s->mark, s->list, depth_counts, fail);
  const unsigned grid = grid_of(blas_nodes);
  for (uint32_t level = 0; level < levels; level++) hipLaunchKernelGGL(k_sched_down, dim3(grid), dim3(REFIT_BLOCK), 0, st, nodes, blas_nodes, s->list, depth_counts, level, s->mark, fail);
  for (uint32_t level = levels; level-- > 0;)
    hipLaunchKernelGGL(k_sched_height, dim3(grid), dim3(REFIT_BLOCK), 0, st, nodes, blas_nodes, s->list, depth_counts, level, s->height, height_counts, levels);
  REFIT_TRY(hipGetLastError());
  REFIT_TRY(hipMemcpyAsync(s->readback, s->counts, count_words * 4, hipMemcpyDeviceToHost, st));
  REFIT_TRY(hipStreamSynchronize(st));
  const uint32_t* dc = s->readback;
  const uint32_t* hc = s->readback + (levels + 1);
  if (s->readback[3 * (size_t)(levels + 1)] != 0) {
    err = "refit: a bottom-level node refers outside the bottom levels";
    return false;
  }
  if (dc[levels] != 0 || hc[levels] != 0) {
    err = "refit: the bottom levels are higher than their bound";
    return false;
  }
  uint64_t total = 0;
  for (uint32_t l = 0; l < levels; l++) total += dc[l];
  if (total > blas_nodes) {
    err = "refit: more nodes reached than there are";
    return false;
  }
  std::vector<uint32_t> offsets(levels + 1, 0u);
  s->height_begin.assign(1, 0u);
  uint32_t run = 0;
  for (uint32_t h = 0; h <= levels; h++) {
    offsets[h] = run;
    run += hc[h];
    if (h < levels) s->height_begin.push_back(run);
  }
  if (run != total) {
    err = "refit: the schedule lost nodes";
    return false;
  }
  while (s->height_begin.size() > 1 && s->height_begin[s->height_begin.size() - 1] == s->height_begin[s->height_begin.size() - 2]) s->height_begin.pop_back();
  s->scheduled = (uint32_t)total;
  REFIT_TRY(hipMemcpyAsync(s->offsets, offsets.data(), offsets.size() * 4, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_sched_scatter, dim3(grid_of(total)), dim3(REFIT_BLOCK), 0, st, s->list, (uint32_t)total, s->height, s->offsets, cursors, s->sched);
  // the cost of the tree as it was built: the same kernel over the triangles as they lie there now, nothing written but the scratch
  launch_refit(s, false, nodes, tris, tri_count, st);
  REFIT_TRY(hipGetLastError());
  REFIT_TRY(hipMemcpyAsync(s->readback, s->out_dev, roots.size() * 2 * sizeof(float4), hipMemcpyDeviceToHost, st));
  REFIT_TRY(hipStreamSynchronize(st));  // (`offsets` goes out of scope)
  s->sah_at_build = sah_of(reinterpret_cast<const float*>(s->readback), roots.size());
  s->valid = true;
  return true;
}

bool refit_gather(DeviceRefit* s, BvhTri* tris, uint32_t tri_count, const sthip_PackedVertexData* vertices, uint32_t vertex_count, const uint8_t* indices, uint64_t indices_bytes, void* stream_,
                  std::string& err) {
  hipStream_t st = (hipStream_t)stream_;
  if (!s || !s->valid) {
    err = "refit: no schedule";
    return false;
  }
  REFIT_TRY(hipEventRecord(s->ev[0], st));
  if (tri_count) {
    static_assert(sizeof(sthip_PackedVertexData) == 32 && sizeof(BvhTri) == 48, "two / three 16-byte words");
    hipLaunchKernelGGL(k_refit_gather, dim3(grid_of(tri_count)), dim3(REFIT_BLOCK), 0, st, reinterpret_cast<float4*>(tris), tri_count, reinterpret_cast<const float4*>(vertices), vertex_count, indices,
                       indices_bytes);
    REFIT_TRY(hipGetLastError());
  }
  return true;
}

bool refit_boxes(DeviceRefit* s, BvhNodeSlot* nodes, const BvhTri* tris, uint32_t tri_count, const sthip_InstanceData* instances, const std::vector<uint32_t>& emitter_instances,
                 const sthip_PackedVertexData* vertices, uint32_t vertex_count, const uint8_t* indices, uint64_t indices_bytes, void* stream_, RefitResult& result, std::string& err) {
  hipStream_t st = (hipStream_t)stream_;
  result = RefitResult();
  if (!s || !s->valid) {
    err = "refit: no schedule";
    return false;
  }
  const size_t roots = s->roots.size(), emitters = emitter_instances.size();
  if (roots + emitters + 1 > s->root_capacity) {
    err = "refit: more emitters than prepared for";
    return false;
  }
  launch_refit(s, true, nodes, tris, tri_count, st);
  if (emitters) {
    REFIT_TRY(hipMemcpyAsync(s->roots_dev + roots, emitter_instances.data(), emitters * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_refit_emitter_boxes, dim3((unsigned)emitters), dim3(REFIT_BLOCK), 0, st, instances, s->roots_dev + roots, reinterpret_cast<const float4*>(vertices), vertex_count, indices, indices_bytes,
                       s->out_dev + 2 * roots);
  }
  REFIT_TRY(hipGetLastError());
  REFIT_TRY(hipEventRecord(s->ev[1], st));
  if (roots + emitters) REFIT_TRY(hipMemcpyAsync(s->readback, s->out_dev, (roots + emitters) * 2 * sizeof(float4), hipMemcpyDeviceToHost, st));
  REFIT_TRY(hipStreamSynchronize(st));
  (void)hipEventElapsedTime(&result.gpu_ms, s->ev[0], s->ev[1]);
  const float* rec = reinterpret_cast<const float*>(s->readback);
  result.root_boxes.assign(rec, rec + 8 * roots);
  result.emitter_boxes.assign(rec + 8 * roots, rec + 8 * (roots + emitters));
  result.sah_cost = sah_of(rec, roots);
  result.sah_cost_at_build = s->sah_at_build;
  return true;
}

}  // namespace sthip
