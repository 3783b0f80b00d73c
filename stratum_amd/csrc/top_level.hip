// top_level.hip — the device side of sthip_scene_set_transforms (top_level.h, sthip.h): derived matrices, entry boxes with the
// host builder's arithmetic, and a radix-tree top level (Karras 2012) over 48-bit Morton keys that carry the entry index in
// their low 16 bits. At most 65 535 entries: launch count and the one read-back decide the time, so everything is enqueued on
// the stream back to back and the host waits once, for the 48-byte result record.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "radix_tree.h"
#include "top_level.h"

namespace sthip {
namespace {

#define TL_BLOCK 256

struct TBox {
  float lo[3], hi[3];
};
struct TNode {  // a fitted inner node of the radix tree
  float lo[3], hi[3];
  uint32_t height, pad;
};
// the head of the scratch: the result record, then the centroid bounds (ordered integers)
struct TlHead {
  TopLevelResult res;
  uint32_t cb[6];
  uint32_t pad[2];
};

__device__ __forceinline__ uint32_t tl_f2ord(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float tl_ord2f(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }
__device__ __forceinline__ float tl_wave_min(float v) {
  for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float tl_wave_max(float v) {
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ void tl_flag(TlHead* head, uint32_t flag, uint32_t index) {
  atomicOr(&head->res.flags, flag);
  atomicMin(&head->res.first_bad, index);
}

__global__ void k_tl_init(TlHead* head) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  TlHead h;
  memset(&h, 0, sizeof(h));
  h.res.first_bad = 0xFFFFFFFFu;
  for (int a = 0; a < 3; a++) {
    h.res.box[a] = h.cb[a] = 0xFFFFFFFFu;  // (ordered: +max; any real value is below)
    h.res.box[3 + a] = h.cb[3 + a] = 0u;
  }
  *head = h;
}

// Per instance: the new transform into the staging, the inverse (given or derived in binary64) and the motion matrix (given,
// the identity, or previous x inverse in binary32); a merged instance must stay the identity.
__global__ void __launch_bounds__(TL_BLOCK) k_derive_transforms(uint32_t n, const sthip_TransformData* xf, const sthip_TransformData* inv, const sthip_TransformData* motion, int derive_motion_flag,
                                                                const sthip_TransformData* resident_xf, const uint8_t* merged, sthip_TransformData* out_xf, sthip_TransformData* out_inv,
                                                                sthip_TransformData* out_motion, TlHead* head) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float m[12], iv[12], mo[12];
  const float* src = &xf[i].m[0][0];
  for (int k = 0; k < 12; k++) m[k] = src[k];
  if (inv) {
    const float* s = &inv[i].m[0][0];
    for (int k = 0; k < 12; k++) iv[k] = s[k];
  } else if (!derive_inverse(m, iv)) {
    tl_flag(head, TL_FLAG_SINGULAR, i);
  }
  if (motion) {
    const float* s = &motion[i].m[0][0];
    for (int k = 0; k < 12; k++) mo[k] = s[k];
  } else if (derive_motion_flag) {
    float prev[12];
    const float* s = &resident_xf[i].m[0][0];
    for (int k = 0; k < 12; k++) prev[k] = s[k];
    derive_motion(prev, iv, mo);
  } else {
    for (int k = 0; k < 12; k++) mo[k] = (k == 0 || k == 5 || k == 10) ? 1.0f : 0.0f;
  }
  if (merged[i] && !(transform_is_identity(m) && transform_is_identity(iv))) tl_flag(head, TL_FLAG_MERGED_MOVED, i);
  float* o = &out_xf[i].m[0][0];
  for (int k = 0; k < 12; k++) o[k] = m[k];
  o = &out_inv[i].m[0][0];
  for (int k = 0; k < 12; k++) o[k] = iv[k];
  o = &out_motion[i].m[0][0];
  for (int k = 0; k < 12; k++) o[k] = mo[k];
}

// Per entry: the new entry record (the inverse of its instance), its exact world box, and the scene box and the bounds of the
// box centres folded per wave into ordered-integer atomics (min / max are exact: the order of the fold changes no bit but
// the sign of a zero).
__global__ void __launch_bounds__(TL_BLOCK) k_entry_boxes(uint32_t m, const TlasEntry* entries, const sthip_TransformData* xf, const sthip_TransformData* inv, uint32_t instance_count,
                                                          const float* obj_box, const DeviceVolume* volumes, uint32_t volume_count, TBox merged_box, TlasEntry* out_entries, TBox* boxes,
                                                          TlHead* head) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  float c[3] = {0, 0, 0};
  const bool live = k < m;
  if (live) {
    TlasEntry e = entries[k];
    float M[12];
    for (int j = 0; j < 12; j++) M[j] = 0.0f;
    bool ok = true;
    if (e.identity != TLAS_ENTRY_IDENTITY) {
      const uint32_t i = e.id_bits;
      if (i < instance_count) {
        const float* s = &xf[i].m[0][0];
        for (int j = 0; j < 12; j++) M[j] = s[j];
        const float* q = &inv[i].m[0][0];
        for (int j = 0; j < 12; j++) e.inv[j] = q[j];
      } else {
        ok = false;
      }
    }
    const DeviceVolume* vol = nullptr;
    if (e.identity == TLAS_ENTRY_VOLUME) {
      if (e.root < volume_count)
        vol = &volumes[e.root];
      else
        ok = false;
    }
    if (ok) {
      float mb[6];
      for (int j = 0; j < 3; j++) {
        mb[j] = merged_box.lo[j];
        mb[3 + j] = merged_box.hi[j];
      }
      entry_world_box(e, M, &obj_box[6 * (size_t)k], vol, mb, lo, hi);
    }
    out_entries[k] = e;
    TBox b;
    bool finite = ok;
    for (int a = 0; a < 3; a++) {
      b.lo[a] = lo[a];
      b.hi[a] = hi[a];
      if (!(fabsf(lo[a]) <= FLT_MAX && fabsf(hi[a]) <= FLT_MAX)) finite = false;
      c[a] = 0.5f * (lo[a] + hi[a]);
    }
    boxes[k] = b;
    // (the merged mesh's kept box is taken as it is, as the host builder takes it: an empty one joins no bound below)
    if (!finite && e.identity != TLAS_ENTRY_IDENTITY) tl_flag(head, TL_FLAG_BOX, k);
    if (!finite) {
      for (int a = 0; a < 3; a++) {  // (keeps the atomics below clear of NaN; the call is refused anyway)
        lo[a] = INFINITY;
        hi[a] = -INFINITY;
      }
    }
  }
  const bool fold = live && lo[0] <= hi[0];
  for (int a = 0; a < 3; a++) {
    const float slo = tl_wave_min(lo[a]), shi = tl_wave_max(hi[a]);
    const float clo = tl_wave_min(fold ? c[a] : INFINITY), chi = tl_wave_max(fold ? c[a] : -INFINITY);
    if ((threadIdx.x & 63u) == 0 && slo <= shi) {
      atomicMin(&head->res.box[a], tl_f2ord(slo));
      atomicMax(&head->res.box[3 + a], tl_f2ord(shi));
      if (clo <= chi) {
        atomicMin(&head->cb[a], tl_f2ord(clo));
        atomicMax(&head->cb[3 + a], tl_f2ord(chi));
      }
    }
  }
}

__device__ __forceinline__ unsigned long long tl_expand16(unsigned long long v) {  // 16 bits -> every third bit
  v &= 0xFFFFull;
  v = (v | v << 16) & 0x0000FF0000FFull;
  v = (v | v << 8) & 0x00F00F00F00Full;
  v = (v | v << 4) & 0x0C30C30C30C3ull;
  v = (v | v << 2) & 0x249249249249ull;
  return v;
}
// key = 48-bit Morton code of the box centre over the centre bounds << 16 | entry: no two keys are equal, and entries with
// equal codes sort by entry index. An axis of zero extent contributes 0.
__global__ void __launch_bounds__(TL_BLOCK) k_tl_keys(uint32_t m, const TBox* boxes, const TlHead* head, unsigned long long* keys) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  unsigned long long code = 0;
  for (int a = 0; a < 3; a++) {
    const float lo = tl_ord2f(head->cb[a]), hi = tl_ord2f(head->cb[3 + a]);
    const float c = 0.5f * (boxes[k].lo[a] + boxes[k].hi[a]);
    const float ext = hi - lo;
    float x = (ext > 0 && ext <= FLT_MAX) ? (c - lo) / ext : 0.0f;
    x = fminf(fmaxf(x * 65536.0f, 0.0f), 65535.0f);  // (fmaxf drops a NaN)
    code |= tl_expand16((unsigned long long)x) << (2 - a);
  }
  keys[k] = (code << 16) | (unsigned long long)k;
}

// Karras 2012 (radix_tree.h, shared with lbvh.hip): one thread per inner node; a child reference is an inner node index or
// 0x80000000 | sorted position
__global__ void __launch_bounds__(TL_BLOCK) k_tl_hierarchy(const unsigned long long* keys, int n, uint32_t* left, uint32_t* right, uint32_t* parent_of_internal, uint32_t* parent_of_leaf) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n - 1) radix_tree_node(keys, n, i, left, right, parent_of_internal, parent_of_leaf);
}

// Bottom-up boxes and heights in one launch, by the arrive counters lbvh.hip uses: the first thread to reach a node stops,
// the second takes the union and goes on. No thread waits for another.
__global__ void __launch_bounds__(TL_BLOCK) k_tl_fit(int n, const unsigned long long* keys, const uint32_t* left, const uint32_t* right, const uint32_t* parent_of_internal,
                                                     const uint32_t* parent_of_leaf, const TBox* boxes, TNode* node_boxes, uint32_t* visits, TlHead* head) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t cur = parent_of_leaf[i];
  for (int guard = 0; guard < 128; guard++) {  // (64-bit distinct keys: the tree is at most 64 high)
    if (cur >= (uint32_t)(n - 1)) return;
    const uint32_t earlier = __hip_atomic_fetch_add(&visits[cur], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (earlier == 0) return;
    const uint32_t c[2] = {left[cur], right[cur]};
    TNode u;
    uint32_t h = 0;
    for (int a = 0; a < 3; a++) {
      u.lo[a] = INFINITY;
      u.hi[a] = -INFINITY;
    }
    for (int s = 0; s < 2; s++) {
      float lo[3], hi[3];
      if (c[s] & 0x80000000u) {
        const TBox b = boxes[(uint32_t)(keys[c[s] & 0x7FFFFFFFu] & 0xFFFFull)];
        for (int a = 0; a < 3; a++) {
          lo[a] = b.lo[a];
          hi[a] = b.hi[a];
        }
      } else {
        const TNode t = node_boxes[c[s]];
        for (int a = 0; a < 3; a++) {
          lo[a] = t.lo[a];
          hi[a] = t.hi[a];
        }
        h = max(h, t.height);
      }
      for (int a = 0; a < 3; a++) {
        u.lo[a] = fminf(u.lo[a], lo[a]);
        u.hi[a] = fmaxf(u.hi[a], hi[a]);
      }
    }
    u.height = 1u + h;
    u.pad = 0;
    node_boxes[cur] = u;
    if (cur == 0) {
      head->res.height = u.height;
      return;
    }
    cur = parent_of_internal[cur];
  }
}

__device__ __forceinline__ void tl_set_child(BvhNode& n, int k, const float lo[3], const float hi[3], uint32_t ref) {
  float* xy = k == 0 ? n.n0xy : n.n1xy;
  xy[0] = lo[0];
  xy[1] = hi[0];
  xy[2] = lo[1];
  xy[3] = hi[1];
  n.nz[2 * k] = lo[2];
  n.nz[2 * k + 1] = hi[2];
  n.ref[k] = ref;
}
// Inner node i of the radix tree -> node blas_nodes + i of the scene's array, unpacked and packed (staging), as flatten lays a
// top level out: inner references offset by blas_nodes, leaves BVH_LEAF_BIT | BVH_INST_BIT | entry
__global__ void __launch_bounds__(TL_BLOCK) k_tl_emit(int n, uint32_t blas_nodes, const unsigned long long* keys, const uint32_t* left, const uint32_t* right, const TBox* boxes, const TNode* node_boxes,
                                                      BvhNode* raw, BvhNodeSlot* packed) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n - 1) return;
  const uint32_t c[2] = {left[i], right[i]};
  BvhNode out;
  memset(&out, 0, sizeof(out));
  for (int s = 0; s < 2; s++) {
    if (c[s] & 0x80000000u) {
      const uint32_t entry = (uint32_t)(keys[c[s] & 0x7FFFFFFFu] & 0xFFFFull);
      const TBox b = boxes[entry];
      tl_set_child(out, s, b.lo, b.hi, BVH_LEAF_BIT | BVH_INST_BIT | entry);
    } else {
      const TNode t = node_boxes[c[s]];
      tl_set_child(out, s, t.lo, t.hi, blas_nodes + c[s]);
    }
  }
  raw[i] = out;
  BvhNodeSlot slot;
  memset(&slot, 0, sizeof(slot));
  slot.n = pack_node(out);
  packed[i] = slot;
}
// One entry: the node that holds its leaf in both slots (bvh_build.cpp: wrap_leaf)
__global__ void k_tl_wrap(const TBox* boxes, BvhNode* raw, BvhNodeSlot* packed, TlHead* head) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const TBox b = boxes[0];
  BvhNode out;
  memset(&out, 0, sizeof(out));
  tl_set_child(out, 0, b.lo, b.hi, BVH_LEAF_BIT | BVH_INST_BIT | 0u);
  tl_set_child(out, 1, b.lo, b.hi, BVH_LEAF_BIT | BVH_INST_BIT | 0u);
  raw[0] = out;
  BvhNodeSlot slot;
  memset(&slot, 0, sizeof(slot));
  slot.n = pack_node(out);
  packed[0] = slot;
  head->res.height = 1;
}

// a device array that grows and keeps its contents' capacity between calls (new memory is poisoned under STHIP_POISON_ALLOC,
// as every buffer of the context is)
template <typename T>
struct TlBuf {
  T* p = nullptr;
  size_t n = 0;
  hipError_t ensure(size_t count) {
    if (count <= n && p) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    if (count == 0) return hipSuccess;
    hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
    if (e == hipSuccess) n = count;
    static const int poison = [] {
      const char* v = getenv("STHIP_POISON_ALLOC");
      return v && *v ? (int)(strtoul(v, nullptr, 0) & 0xFFu) : -1;
    }();
    if (e == hipSuccess && poison >= 0) e = hipMemset(p, poison, count * sizeof(T));
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
};
}  // namespace

struct DeviceTopLevel {
  TlBuf<TlHead> head;
  TlBuf<uint8_t> merged;
  TlBuf<float> obj_box;
  TlBuf<sthip_TransformData> xf, inv, motion;  // staging: the new matrices
  TlBuf<TlasEntry> entries;                    // staging: the new entries
  TlBuf<TBox> boxes;
  TlBuf<unsigned long long> keys, keys_sorted;
  TlBuf<uint32_t> left, right, parent_of_internal, parent_of_leaf, visits;
  TlBuf<TNode> node_boxes;
  TlBuf<BvhNode> raw;
  TlBuf<BvhNodeSlot> packed;
  TlBuf<uint8_t> sort_tmp;
  hipEvent_t ev[2] = {nullptr, nullptr};
  uint32_t static_instances = 0, static_entries = 0;
  // what the staging holds since the last top_level_build
  uint32_t staged_instances = 0, staged_entries = 0, staged_nodes = 0, staged_blas_nodes = 0;
};

DeviceTopLevel* device_top_level_create() { return new DeviceTopLevel(); }
void device_top_level_destroy(DeviceTopLevel* tl) {
  if (!tl) return;
  tl->head.release();
  tl->merged.release();
  tl->obj_box.release();
  tl->xf.release();
  tl->inv.release();
  tl->motion.release();
  tl->entries.release();
  tl->boxes.release();
  tl->keys.release();
  tl->keys_sorted.release();
  tl->left.release();
  tl->right.release();
  tl->parent_of_internal.release();
  tl->parent_of_leaf.release();
  tl->visits.release();
  tl->node_boxes.release();
  tl->raw.release();
  tl->packed.release();
  tl->sort_tmp.release();
  for (int k = 0; k < 2; k++)
    if (tl->ev[k]) (void)hipEventDestroy(tl->ev[k]);
  delete tl;
}

#define TL_TRY(expr)                                                        \
  do {                                                                      \
    const hipError_t e_ = (expr);                                           \
    if (e_ != hipSuccess) {                                                 \
      err = std::string("top level: ") + hipGetErrorString(e_) + " (" #expr ")"; \
      return false;                                                         \
    }                                                                       \
  } while (0)

bool top_level_set_static(DeviceTopLevel* tl, const uint8_t* merged, uint32_t instance_count, const float* obj_box, uint32_t entry_count, void* stream_, std::string& err) {
  hipStream_t stream = (hipStream_t)stream_;
  TL_TRY(tl->merged.ensure(std::max<size_t>(1, instance_count)));
  TL_TRY(tl->obj_box.ensure(std::max<size_t>(6, 6 * (size_t)entry_count)));
  TL_TRY(hipStreamSynchronize(stream));  // (a launch of an earlier call may still read the tables)
  if (instance_count) TL_TRY(hipMemcpy(tl->merged.p, merged, instance_count, hipMemcpyHostToDevice));
  if (entry_count) TL_TRY(hipMemcpy(tl->obj_box.p, obj_box, 6 * (size_t)entry_count * sizeof(float), hipMemcpyHostToDevice));
  tl->static_instances = instance_count;
  tl->static_entries = entry_count;
  return true;
}

static inline uint32_t tl_grid(uint32_t n) { return std::max(1u, (n + TL_BLOCK - 1) / TL_BLOCK); }

bool top_level_build(DeviceTopLevel* tl, const TopLevelInputs& in, void* stream_, TopLevelResult& result, float& gpu_ms, std::string& err) {
  hipStream_t stream = (hipStream_t)stream_;
  const uint32_t n = in.instance_count, m = in.entry_count;
  gpu_ms = 0;
  if (tl->static_instances != n || tl->static_entries != m) {
    err = "top level: the static tables do not belong to this scene";
    return false;
  }
  // ---- reserve ----
  TL_TRY(tl->head.ensure(1));
  TL_TRY(tl->xf.ensure(std::max(1u, n)));
  TL_TRY(tl->inv.ensure(std::max(1u, n)));
  TL_TRY(tl->motion.ensure(std::max(1u, n)));
  TL_TRY(tl->entries.ensure(std::max(1u, m)));
  TL_TRY(tl->boxes.ensure(std::max(1u, m)));
  const bool tree = in.build_tree && m >= 2;
  size_t tmp_bytes = 0;
  if (tree) {
    TL_TRY(tl->keys.ensure(m));
    TL_TRY(tl->keys_sorted.ensure(m));
    TL_TRY(tl->left.ensure(m));
    TL_TRY(tl->right.ensure(m));
    TL_TRY(tl->parent_of_internal.ensure(m));
    TL_TRY(tl->parent_of_leaf.ensure(m));
    TL_TRY(tl->visits.ensure(m));
    TL_TRY(tl->node_boxes.ensure(m));
    TL_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, tl->keys.p, tl->keys_sorted.p, (int)m, 0, 64, stream));
    TL_TRY(tl->sort_tmp.ensure(std::max<size_t>(16, tmp_bytes)));
  }
  if (in.build_tree && m >= 1) {
    TL_TRY(tl->raw.ensure(std::max(1u, m)));
    TL_TRY(tl->packed.ensure(std::max(1u, m)));
  }
  for (int k = 0; k < 2; k++)
    if (!tl->ev[k]) TL_TRY(hipEventCreate(&tl->ev[k]));
  // ---- enqueue ----
  TL_TRY(hipEventRecord(tl->ev[0], stream));
  TBox merged_box;
  for (int a = 0; a < 3; a++) {
    merged_box.lo[a] = in.merged_box[a];
    merged_box.hi[a] = in.merged_box[3 + a];
  }
  hipLaunchKernelGGL(k_tl_init, dim3(1), dim3(64), 0, stream, tl->head.p);
  if (n)
    hipLaunchKernelGGL(k_derive_transforms, dim3(tl_grid(n)), dim3(TL_BLOCK), 0, stream, n, in.xf, in.inv, in.motion, in.derive_motion ? 1 : 0, in.resident_xf, tl->merged.p, tl->xf.p, tl->inv.p,
                       tl->motion.p, tl->head.p);
  if (m)
    hipLaunchKernelGGL(k_entry_boxes, dim3(tl_grid(m)), dim3(TL_BLOCK), 0, stream, m, in.entries, tl->xf.p, tl->inv.p, n, tl->obj_box.p, in.volumes, in.volume_count, merged_box, tl->entries.p, tl->boxes.p,
                       tl->head.p);
  tl->staged_nodes = 0;
  if (tree) {
    hipLaunchKernelGGL(k_tl_keys, dim3(tl_grid(m)), dim3(TL_BLOCK), 0, stream, m, tl->boxes.p, tl->head.p, tl->keys.p);
    // (the distinct 64-bit keys are sorted whole, the entry index included: the order of equal codes does not rest on the sort)
    TL_TRY(hipcub::DeviceRadixSort::SortKeys(tl->sort_tmp.p, tmp_bytes, tl->keys.p, tl->keys_sorted.p, (int)m, 0, 64, stream));
    TL_TRY(hipMemsetAsync(tl->visits.p, 0, (size_t)m * sizeof(uint32_t), stream));
    hipLaunchKernelGGL(k_tl_hierarchy, dim3(tl_grid(m - 1)), dim3(TL_BLOCK), 0, stream, tl->keys_sorted.p, (int)m, tl->left.p, tl->right.p, tl->parent_of_internal.p, tl->parent_of_leaf.p);
    hipLaunchKernelGGL(k_tl_fit, dim3(tl_grid(m)), dim3(TL_BLOCK), 0, stream, (int)m, tl->keys_sorted.p, tl->left.p, tl->right.p, tl->parent_of_internal.p, tl->parent_of_leaf.p, tl->boxes.p,
                       tl->node_boxes.p, tl->visits.p, tl->head.p);
    hipLaunchKernelGGL(k_tl_emit, dim3(tl_grid(m - 1)), dim3(TL_BLOCK), 0, stream, (int)m, in.blas_nodes, tl->keys_sorted.p, tl->left.p, tl->right.p, tl->boxes.p, tl->node_boxes.p, tl->raw.p,
                       tl->packed.p);
    tl->staged_nodes = m - 1;
  } else if (in.build_tree && m == 1) {
    hipLaunchKernelGGL(k_tl_wrap, dim3(1), dim3(64), 0, stream, tl->boxes.p, tl->raw.p, tl->packed.p, tl->head.p);
    tl->staged_nodes = 1;
  }
  TL_TRY(hipGetLastError());
  TL_TRY(hipEventRecord(tl->ev[1], stream));
  // ---- the one read-back ----
  TL_TRY(hipMemcpyAsync(&result, &tl->head.p->res, sizeof(TopLevelResult), hipMemcpyDeviceToHost, stream));
  TL_TRY(hipStreamSynchronize(stream));
  (void)hipEventElapsedTime(&gpu_ms, tl->ev[0], tl->ev[1]);
  tl->staged_instances = n;
  tl->staged_entries = m;
  tl->staged_blas_nodes = in.blas_nodes;
  return true;
}

bool top_level_install(DeviceTopLevel* tl, sthip_TransformData* xf, sthip_TransformData* inv, sthip_TransformData* motion, TlasEntry* entries, BvhNodeSlot* nodes, void* stream_, std::string& err) {
  hipStream_t stream = (hipStream_t)stream_;
  const size_t n = tl->staged_instances, m = tl->staged_entries;
  if (n && xf) TL_TRY(hipMemcpyAsync(xf, tl->xf.p, n * sizeof(sthip_TransformData), hipMemcpyDeviceToDevice, stream));
  if (n && inv) TL_TRY(hipMemcpyAsync(inv, tl->inv.p, n * sizeof(sthip_TransformData), hipMemcpyDeviceToDevice, stream));
  if (n && motion) TL_TRY(hipMemcpyAsync(motion, tl->motion.p, n * sizeof(sthip_TransformData), hipMemcpyDeviceToDevice, stream));
  if (m && entries) TL_TRY(hipMemcpyAsync(entries, tl->entries.p, m * sizeof(TlasEntry), hipMemcpyDeviceToDevice, stream));
  if (tl->staged_nodes && nodes) TL_TRY(hipMemcpyAsync(nodes, tl->packed.p, (size_t)tl->staged_nodes * sizeof(BvhNodeSlot), hipMemcpyDeviceToDevice, stream));
  return true;
}

bool top_level_read_boxes(DeviceTopLevel* tl, float* boxes, uint32_t entry_count, void* stream_, std::string& err) {
  hipStream_t stream = (hipStream_t)stream_;
  if (entry_count > tl->staged_entries) {
    err = "top level: no boxes staged";
    return false;
  }
  if (entry_count) TL_TRY(hipMemcpyAsync(boxes, tl->boxes.p, (size_t)entry_count * sizeof(TBox), hipMemcpyDeviceToHost, stream));
  TL_TRY(hipStreamSynchronize(stream));
  return true;
}
bool top_level_read_nodes(DeviceTopLevel* tl, BvhNode* nodes, uint32_t node_count, void* stream_, std::string& err) {
  hipStream_t stream = (hipStream_t)stream_;
  if (node_count > tl->staged_nodes) {
    err = "top level: no nodes staged";
    return false;
  }
  if (node_count) TL_TRY(hipMemcpyAsync(nodes, tl->raw.p, (size_t)node_count * sizeof(BvhNode), hipMemcpyDeviceToHost, stream));
  TL_TRY(hipStreamSynchronize(stream));
  return true;
}

}  // namespace sthip
