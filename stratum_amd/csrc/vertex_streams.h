// vertex_streams.h — sthip_scene_set_vertices on the device (vertex_streams.hip): strided position / normal / uv streams packed
// into the resident gVertices, and shading normals made again from the moved positions (sthip.h holds both contracts).
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/sthip.h"
#include "scene_prepare.h"

namespace sthip {

// The streams of one call as the kernels read them: device pointers, 4-byte aligned, strides in bytes (a NULL stream is absent)
struct VertexStreams {
  const void* positions = nullptr;
  const void* normals = nullptr;
  const void* texcoords = nullptr;
  uint32_t position_stride = 0, normal_stride = 0, texcoord_stride = 0;
  uint32_t first_vertex = 0, vertex_count = 0;
};

// Enqueues k_pack_vertices (nothing for an empty range): record first_vertex + i of `vertices` becomes
// {positions[i], u, normals[i], v}, bit copies; the fields of an absent stream and every record outside the range are not written.
bool pack_vertices_launch(sthip_PackedVertexData* vertices, const VertexStreams& s, void* stream, std::string& err);

// The corners of the scene's meshes grouped by the vertex they name, made once per uploaded topology and kept until the next
// upload: row v holds the triangle slots of the corners whose absolute index is v, in ascending (mesh, triangle, corner).
struct DeviceVertexAdjacency;
DeviceVertexAdjacency* device_vertex_adjacency_create();
void device_vertex_adjacency_destroy(DeviceVertexAdjacency*);
void device_vertex_adjacency_invalidate(DeviceVertexAdjacency*);  // another scene is resident now: made again at the next prepare
// Makes the adjacency of `meshes` (scene_prepare.h: list_vertex_meshes, in its order) over the resident index buffer if it is
// not the valid one, and the scratch of the face vectors. Reads gIndices only; every allocation of a normal pass happens here.
// `built`: the adjacency was made by this call.
bool vertex_adjacency_prepare(DeviceVertexAdjacency*, const std::vector<VertexMesh>& meshes, const uint8_t* indices, uint64_t indices_bytes, uint32_t vertex_count, void* stream, bool& built, std::string& err);
bool vertex_adjacency_valid(const DeviceVertexAdjacency*);
// Enqueues k_face_vectors over every triangle of the meshes and k_vertex_normals over [first_vertex, first_vertex + count):
// the normal contract of sthip.h. `between` (a hipEvent_t, or NULL): recorded between the two launches (measurement only).
bool vertex_normals_launch(DeviceVertexAdjacency*, sthip_PackedVertexData* vertices, uint32_t vertex_count, const uint8_t* indices, uint64_t indices_bytes, uint32_t first_vertex, uint32_t count, void* stream,
                           void* between, std::string& err);

}  // namespace sthip
