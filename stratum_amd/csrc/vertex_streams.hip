// vertex_streams.hip — vertices from device memory (sthip_scene_set_vertices, api.hip): strided position / normal / uv streams
// are packed into the resident gVertices, and the shading normals of the written range are made again from the moved
// positions. The gather, the refit and the top level of refit.hip follow unchanged.
//
// The reference packs in kernels/copy_vertices.hlsl (PackedVertexData::set, :29-37): one thread per vertex reads the three
// streams at their strides and writes {position, u, normal, v}. k_pack_vertices is that pass with absent streams allowed: one
// lane per vertex, 4-byte loads (a stream is only 4-byte aligned), and a 16-byte store for each half of the record whose four
// words the lane knows; of a half it knows in part it writes only its own words, so the resident bits of the rest stay.
//
// The reference has no pass that makes normals for moved positions (anim.hlsl blends and skins given ones). Here they are
// the normalised sum of the area-weighted face vectors around a vertex, in an order that is part of the contract (sthip.h),
// so that the result is the same bytes on every run and on the host's restatement. A sum that must be reproducible is made
// store-then-sum: k_face_vectors leaves the cross product of every triangle of the scene's meshes in a 16-byte slot of a
// scratch array (three index loads, three position loads); k_vertex_normals, one lane per vertex of the range, walks the
// vertex's row of the adjacency, adds the slots in the row's order, normalises and writes 12 bytes. No float atomics, no flag
// or spin inside a launch: stream order between the launches is the only ordering, as in refit.hip.
//
// The adjacency belongs to the index buffer, not to the positions: it is made once per uploaded topology. Every corner
// (mesh m, triangle t, corner c) gets the serial 3 * (triangles of the meshes before m + t) + c, which ascends as (m, t, c)
// does; the 64-bit keys (absolute vertex << 32) | serial are sorted (radix sort); row v starts at the first key that is not
// below v << 32 (a binary search per vertex: integers only, no atomics), and the row's entries are the slots serial / 3.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "vertex_streams.h"

namespace sthip {

namespace {
// one mesh with triangles as the kernels see it
struct DeviceMesh {
  uint32_t indices_byte_offset, first_vertex, index_stride;
  uint32_t tri_base;  // triangles of the meshes before this one
};
}  // namespace

struct DeviceVertexAdjacency {
  bool valid = false;
  uint32_t mesh_count = 0, tri_count = 0, vertex_count = 0;
  DeviceMesh* meshes = nullptr;
  uint32_t* rows = nullptr;   // vertex_count + 1: row v is [rows[v], rows[v + 1]) of `slots`
  uint32_t* slots = nullptr;  // 3 per triangle: the triangle slot of each corner, grouped by vertex
  float4* faces = nullptr;    // 1 per triangle: (g.xyz, 0), written by every call before it is read
  size_t mesh_capacity = 0, row_capacity = 0, tri_capacity = 0;
};

DeviceVertexAdjacency* device_vertex_adjacency_create() { return new DeviceVertexAdjacency(); }
void device_vertex_adjacency_invalidate(DeviceVertexAdjacency* a) {
  if (a) a->valid = false;
}
bool vertex_adjacency_valid(const DeviceVertexAdjacency* a) { return a && a->valid; }
void device_vertex_adjacency_destroy(DeviceVertexAdjacency* a) {
  if (!a) return;
  (void)hipFree(a->meshes);
  (void)hipFree(a->rows);
  (void)hipFree(a->slots);
  (void)hipFree(a->faces);
  delete a;
}

namespace {

constexpr unsigned VS_BLOCK = 256;

// tests: STHIP_POISON_ALLOC=<byte> (context.h, DevBuf::ensure) fills every new buffer of this file too
int poison_byte() {
  static const int poison = [] {
    const char* v = getenv("STHIP_POISON_ALLOC");
    return v && *v ? (int)(strtoul(v, nullptr, 0) & 0xFFu) : -1;
  }();
  return poison;
}
template <typename T>
hipError_t vs_malloc(T** p, size_t bytes) {
  hipError_t e = hipMalloc((void**)p, bytes);
  if (e == hipSuccess && poison_byte() >= 0) e = hipMemset(*p, poison_byte(), bytes);
  return e;
}
// scratch of the adjacency's construction: freed when the function that made it returns, however it returns
struct Scratch {
  void* p = nullptr;
  ~Scratch() {
    if (p) (void)hipFree(p);
  }
};

inline unsigned grid_of(size_t n) { return (unsigned)std::max<size_t>(1, (n + VS_BLOCK - 1) / VS_BLOCK); }

// ---- pack ----
struct PackArgs {
  uint4* vertices;  // gVertices + first_vertex: 2 per record
  const uint8_t* positions;
  const uint8_t* normals;
  const uint8_t* texcoords;
  uint32_t position_stride, normal_stride, texcoord_stride, vertex_count;
};

__global__ void __launch_bounds__(VS_BLOCK) k_pack_vertices(const PackArgs a) {
  const uint32_t i = blockIdx.x * VS_BLOCK + threadIdx.x;
  if (i >= a.vertex_count) return;
  const uint32_t* p = reinterpret_cast<const uint32_t*>(a.positions + (size_t)i * a.position_stride);
  const uint32_t px = p[0], py = p[1], pz = p[2];
  uint32_t u = 0, v = 0, nx = 0, ny = 0, nz = 0;
  const bool has_uv = a.texcoords != nullptr, has_n = a.normals != nullptr;  // (uniform over the launch)
  if (has_uv) {
    const uint32_t* t = reinterpret_cast<const uint32_t*>(a.texcoords + (size_t)i * a.texcoord_stride);
    u = t[0], v = t[1];
  }
  if (has_n) {
    const uint32_t* n = reinterpret_cast<const uint32_t*>(a.normals + (size_t)i * a.normal_stride);
    nx = n[0], ny = n[1], nz = n[2];
  }
  uint4* rec = a.vertices + 2 * (size_t)i;  // (32-byte aligned)
  uint32_t* words = reinterpret_cast<uint32_t*>(rec);
  if (has_uv) {
    rec[0] = make_uint4(px, py, pz, u);
  } else {
    *reinterpret_cast<uint2*>(words) = make_uint2(px, py);
    words[2] = pz;
  }
  if (has_n && has_uv) {
    rec[1] = make_uint4(nx, ny, nz, v);
  } else if (has_n) {
    *reinterpret_cast<uint2*>(words + 4) = make_uint2(nx, ny);
    words[6] = nz;
  } else if (has_uv) {
    words[7] = v;
  }
}

// ---- the corners of the meshes ----
// the mesh of triangle slot t: the last one whose tri_base is not above t (no mesh of the table is empty)
__device__ inline DeviceMesh mesh_of(const DeviceMesh* meshes, uint32_t mesh_count, uint32_t t) {
  uint32_t lo = 0, hi = mesh_count;  // meshes[lo].tri_base <= t < meshes[hi].tri_base
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (meshes[mid].tri_base <= t)
      lo = mid;
    else
      hi = mid;
  }
  return meshes[lo];
}
// The three absolute indices of triangle slot t, read as refit.hip reads them: byte loads (an index buffer's byte offset need
// not be aligned to its stride), zero-extended, plus first_vertex. false: the triple lies outside gIndices or names a vertex
// that is not resident (the builders have refused such scenes already).
__device__ inline bool corner_indices(const DeviceMesh& m, uint32_t t, const uint8_t* indices, uint64_t indices_bytes, uint32_t vertex_count, uint32_t idx[3]) {
  const uint32_t stride = m.index_stride == 2u ? 2u : 4u;
  const uint64_t at = (uint64_t)m.indices_byte_offset + (uint64_t)(t - m.tri_base) * 3u * stride;
  if (at + 3u * stride > indices_bytes) return false;
  bool ok = true;
  for (int k = 0; k < 3; k++) {
    const uint8_t* q = indices + at + (size_t)k * stride;
    const uint32_t raw = stride == 2u ? ((uint32_t)q[0] | (uint32_t)q[1] << 8) : ((uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24);
    const uint64_t abs_index = (uint64_t)raw + m.first_vertex;
    ok = ok && abs_index < vertex_count;
    idx[k] = (uint32_t)abs_index;
  }
  return ok;
}

// a corner of a triple that cannot be read sorts behind every vertex: no row holds it
__global__ void __launch_bounds__(VS_BLOCK) k_adjacency_keys(const DeviceMesh* meshes, uint32_t mesh_count, uint32_t tri_count, const uint8_t* indices, uint64_t indices_bytes, uint32_t vertex_count,
                                                             unsigned long long* keys) {
  const uint32_t t = blockIdx.x * VS_BLOCK + threadIdx.x;
  if (t >= tri_count) return;
  const DeviceMesh m = mesh_of(meshes, mesh_count, t);
  uint32_t idx[3];
  const bool ok = corner_indices(m, t, indices, indices_bytes, vertex_count, idx);
  for (uint32_t c = 0; c < 3u; c++) keys[3 * (size_t)t + c] = ((unsigned long long)(ok ? idx[c] : 0xFFFFFFFFu) << 32) | (unsigned long long)(3u * t + c);
}
// row v starts at the first sorted key that is not below v << 32; rows[vertex_count] ends the last row
__global__ void __launch_bounds__(VS_BLOCK) k_adjacency_rows(const unsigned long long* sorted, uint32_t corner_count, uint32_t vertex_count, uint32_t* rows) {
  const uint32_t v = blockIdx.x * VS_BLOCK + threadIdx.x;
  if (v > vertex_count) return;
  const unsigned long long bound = (unsigned long long)v << 32;
  uint32_t lo = 0, hi = corner_count;  // every key before lo is below the bound, none from hi on is
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (sorted[mid] < bound)
      lo = mid + 1u;
    else
      hi = mid;
  }
  rows[v] = lo;
}
__global__ void __launch_bounds__(VS_BLOCK) k_adjacency_slots(const unsigned long long* sorted, uint32_t corner_count, uint32_t* slots) {
  const uint32_t i = blockIdx.x * VS_BLOCK + threadIdx.x;
  if (i >= corner_count) return;
  slots[i] = (uint32_t)(sorted[i] & 0xFFFFFFFFull) / 3u;
}

// ---- normals ----
__global__ void __launch_bounds__(VS_BLOCK) k_face_vectors(const DeviceMesh* meshes, uint32_t mesh_count, uint32_t tri_count, const uint8_t* indices, uint64_t indices_bytes, const float4* vertices,
                                                           uint32_t vertex_count, float4* faces) {
  const uint32_t t = blockIdx.x * VS_BLOCK + threadIdx.x;
  if (t >= tri_count) return;
  const DeviceMesh m = mesh_of(meshes, mesh_count, t);
  uint32_t idx[3];
  if (!corner_indices(m, t, indices, indices_bytes, vertex_count, idx)) {  // (no row holds its corners)
    faces[t] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  const float4 p0 = vertices[2 * (size_t)idx[0]], p1 = vertices[2 * (size_t)idx[1]], p2 = vertices[2 * (size_t)idx[2]];  // position.xyz | u
  const float e1x = p1.x - p0.x, e1y = p1.y - p0.y, e1z = p1.z - p0.z;
  const float e2x = p2.x - p0.x, e2y = p2.y - p0.y, e2z = p2.z - p0.z;
  // (-ffp-contract=off: every product is rounded before the subtraction)
  faces[t] = make_float4(e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x, 0.0f);
}

__global__ void __launch_bounds__(VS_BLOCK) k_vertex_normals(const uint32_t* rows, const uint32_t* slots, const float4* faces, float4* vertices, uint32_t first_vertex, uint32_t count) {
  const uint32_t i = blockIdx.x * VS_BLOCK + threadIdx.x;
  if (i >= count) return;
  const uint32_t v = first_vertex + i;
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  for (uint32_t k = rows[v], end = rows[v + 1]; k < end; k++) {
    const float4 g = faces[slots[k]];
    sx = sx + g.x, sy = sy + g.y, sz = sz + g.z;
  }
  const float d = sx * sx + sy * sy + sz * sz;  // dot3 of device_math.h: left to right
  if (!(d > 0.0f && d < __builtin_inff())) return;  // the resident normal stays
  const float inv = 1.0f / sqrtf(d);
  float* n = reinterpret_cast<float*>(vertices + 2 * (size_t)v + 1);  // (16-byte aligned; the fourth word is v and stays)
  *reinterpret_cast<float2*>(n) = make_float2(sx * inv, sy * inv);
  n[2] = sz * inv;
}

}  // namespace

#define VS_TRY(x)                                           \
  do {                                                      \
    const hipError_t e_ = (x);                              \
    if (e_ != hipSuccess) {                                 \
      err = std::string(#x) + ": " + hipGetErrorString(e_); \
      return false;                                         \
    }                                                       \
  } while (0)

bool pack_vertices_launch(sthip_PackedVertexData* vertices, const VertexStreams& s, void* stream, std::string& err) {
  static_assert(sizeof(sthip_PackedVertexData) == 32, "two 16-byte words");
  if (!s.vertex_count) return true;
  if (!s.positions) {
    err = "k_pack_vertices: no positions";
    return false;
  }
  PackArgs a{};
  a.vertices = reinterpret_cast<uint4*>(vertices + s.first_vertex);
  a.positions = static_cast<const uint8_t*>(s.positions);
  a.normals = static_cast<const uint8_t*>(s.normals);
  a.texcoords = static_cast<const uint8_t*>(s.texcoords);
  a.position_stride = s.position_stride;
  a.normal_stride = s.normal_stride;
  a.texcoord_stride = s.texcoord_stride;
  a.vertex_count = s.vertex_count;
  hipLaunchKernelGGL(k_pack_vertices, dim3(grid_of(s.vertex_count)), dim3(VS_BLOCK), 0, (hipStream_t)stream, a);
  VS_TRY(hipGetLastError());
  return true;
}

bool vertex_adjacency_prepare(DeviceVertexAdjacency* a, const std::vector<VertexMesh>& meshes, const uint8_t* indices, uint64_t indices_bytes, uint32_t vertex_count, void* stream, bool& built, std::string& err) {
  built = false;
  if (a->valid && a->vertex_count == vertex_count) return true;
  a->valid = false;
  hipStream_t st = (hipStream_t)stream;
  std::vector<DeviceMesh> table;
  uint64_t tris = 0;
  for (const VertexMesh& m : meshes) {
    if (!m.prim_count) continue;
    table.push_back(DeviceMesh{m.indices_byte_offset, m.first_vertex, m.index_stride, (uint32_t)tris});
    tris += m.prim_count;
    if (3 * tris > 0x7FFFFFFFull) {
      err = "the meshes have more than 2^31 corners";
      return false;
    }
  }
  const uint32_t T = (uint32_t)tris, C = 3u * T;
  if (table.size() > a->mesh_capacity || !a->meshes) {
    (void)hipFree(a->meshes);
    a->meshes = nullptr, a->mesh_capacity = 0;
    VS_TRY(vs_malloc(&a->meshes, std::max<size_t>(1, table.size()) * sizeof(DeviceMesh)));
    a->mesh_capacity = std::max<size_t>(1, table.size());
  }
  if ((size_t)vertex_count + 1 > a->row_capacity || !a->rows) {
    (void)hipFree(a->rows);
    a->rows = nullptr, a->row_capacity = 0;
    VS_TRY(vs_malloc(&a->rows, ((size_t)vertex_count + 1) * sizeof(uint32_t)));
    a->row_capacity = (size_t)vertex_count + 1;
  }
  if (T > a->tri_capacity || !a->slots || !a->faces) {
    (void)hipFree(a->slots);
    (void)hipFree(a->faces);
    a->slots = nullptr, a->faces = nullptr, a->tri_capacity = 0;
    VS_TRY(vs_malloc(&a->slots, std::max<size_t>(1, C) * sizeof(uint32_t)));
    VS_TRY(vs_malloc(&a->faces, std::max<size_t>(1, T) * sizeof(float4)));
    a->tri_capacity = T;
  }
  Scratch keys, sorted, tmp;
  size_t tmp_bytes = 0;
  if (C) {
    VS_TRY(vs_malloc(&keys.p, (size_t)C * 8));
    VS_TRY(vs_malloc(&sorted.p, (size_t)C * 8));
    VS_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, (const unsigned long long*)keys.p, (unsigned long long*)sorted.p, (int)C, 0, 64, st));
    VS_TRY(vs_malloc(&tmp.p, std::max<size_t>(16, tmp_bytes)));
    VS_TRY(hipMemcpyAsync(a->meshes, table.data(), table.size() * sizeof(DeviceMesh), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_adjacency_keys, dim3(grid_of(T)), dim3(VS_BLOCK), 0, st, a->meshes, (uint32_t)table.size(), T, indices, indices_bytes, vertex_count, (unsigned long long*)keys.p);
    VS_TRY(hipGetLastError());
    VS_TRY(hipcub::DeviceRadixSort::SortKeys(tmp.p, tmp_bytes, (const unsigned long long*)keys.p, (unsigned long long*)sorted.p, (int)C, 0, 64, st));
    hipLaunchKernelGGL(k_adjacency_slots, dim3(grid_of(C)), dim3(VS_BLOCK), 0, st, (const unsigned long long*)sorted.p, C, a->slots);
    VS_TRY(hipGetLastError());
  }
  // (without corners every row is empty: the search finds 0 everywhere and reads no key)
  hipLaunchKernelGGL(k_adjacency_rows, dim3(grid_of((size_t)vertex_count + 1)), dim3(VS_BLOCK), 0, st, (const unsigned long long*)sorted.p, C, vertex_count, a->rows);
  VS_TRY(hipGetLastError());
  VS_TRY(hipStreamSynchronize(st));  // (the table is a local of this function, and so is the scratch the launches read)
  a->mesh_count = (uint32_t)table.size();
  a->tri_count = T;
  a->vertex_count = vertex_count;
  a->valid = true;
  built = true;
  return true;
}

bool vertex_normals_launch(DeviceVertexAdjacency* a, sthip_PackedVertexData* vertices, uint32_t vertex_count, const uint8_t* indices, uint64_t indices_bytes, uint32_t first_vertex, uint32_t count, void* stream,
                           void* between, std::string& err) {
  if (!a || !a->valid || a->vertex_count != vertex_count) {
    err = "vertex normals: no adjacency for the resident scene";
    return false;
  }
  if ((uint64_t)first_vertex + count > vertex_count) {
    err = "vertex normals: the range ends past the resident vertices";
    return false;
  }
  hipStream_t st = (hipStream_t)stream;
  if (!count || !a->tri_count) {  // (no triangle names a vertex: every normal stays)
    if (between) VS_TRY(hipEventRecord((hipEvent_t)between, st));
    return true;
  }
  float4* words = reinterpret_cast<float4*>(vertices);
  hipLaunchKernelGGL(k_face_vectors, dim3(grid_of(a->tri_count)), dim3(VS_BLOCK), 0, st, a->meshes, a->mesh_count, a->tri_count, indices, indices_bytes, words, vertex_count, a->faces);
  VS_TRY(hipGetLastError());
  if (between) VS_TRY(hipEventRecord((hipEvent_t)between, st));
  hipLaunchKernelGGL(k_vertex_normals, dim3(grid_of(count)), dim3(VS_BLOCK), 0, st, a->rows, a->slots, a->faces, words, first_vertex, count);
  VS_TRY(hipGetLastError());
  return true;
}

}  // namespace sthip
