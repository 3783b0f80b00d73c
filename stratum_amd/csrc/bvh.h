// bvh.h — acceleration-structure layout in HBM (product-internal; replaces the driver-built
// BLAS/TLAS of src/Core/AccelerationStructure.cpp:5-27 and src/Node/Scene.cpp:435-459,614-629).
//
// One flat array of BVH2 nodes holds the top level and every bottom level. The builders work on the 64-byte BvhNode
// below; what is uploaded is its 48-byte packed form (BvhNodePacked further down). A node stores
// the boxes of its two children in the Aila-Laine arrangement:
//     n0xy = (c0.lo.x, c0.hi.x, c0.lo.y, c0.hi.y)
//     n1xy = (c1.lo.x, c1.hi.x, c1.lo.y, c1.hi.y)
//     nz   = (c0.lo.z, c0.hi.z, c1.lo.z, c1.hi.z)
//     ref  = (child0, child1, 0, 0)
// Child references: bit31 = 0 -> index of an inner node; bit31 = 1 -> leaf:
//     bit30 = 0: triangle leaf, bits[29:2] = first triangle, bits[1:0] = count-1
//     bit30 = 1: instance leaf, bits[15:0] = index into the TLAS entry table
// Leaf triangles are stored in leaf order, 48 bytes each: three float4 (v0, v1, v2 in the object
// space of their mesh); v0.w carries the hit id bits: instance | primitive << 16 for the merged
// world-space mesh, primitive << 16 for a shared mesh (the instance comes from the TLAS entry).
#pragma once
#include <stdint.h>

#define BVH_LEAF_BIT 0x80000000u
#define BVH_INST_BIT 0x40000000u
#define BVH_TOP_BIT 0x40000000u  // on an INNER reference (bit31 = 0): index into the treetop copy (bvh_build.h), not the node array
#define BVH_MAX_LEAF_TRIS 2  // measured on the 1M-triangle atrium: 2 beats 1, 3 and 4 (the leaf reference can encode up to 4)
#define BVH_INVALID_REF 0xFFFFFFFFu  // empty child (never intersected: box is inverted)

struct BvhNode {
  float n0xy[4];
  float n1xy[4];
  float nz[4];
  uint32_t ref[4];
};

struct BvhTri {
  float v0[3];
  uint32_t id;
  float v1[3];
  uint32_t src_indices;  // where the triangle came from: byte offset of its index triple in gIndices
  float v2[3];
  uint32_t src_vertex;   // ... first_vertex of its mesh, bit31 = 32-bit indices (k_fill_tri_shade reads the vertices again through these)
};
// Beside every leaf triangle, in the same order: what shading needs of its three vertices apart from the positions BvhTri
// holds — normal and v of each, the three u (sthip_PackedVertexData: position.xyz u | normal.xyz v). Filled on the device
// once the tree is resident (api.hip: k_fill_tri_shade), whoever built it.
struct BvhTriShade {
  float n0[3], v0;
  float n1[3], v1;
  float n2[3], v2;
  float u[3], pad;
};
// The node as it lies in HBM (and in the LDS treetop): 48 bytes = three float4, so a lane fetches it with THREE 16-byte
// loads. The traversal kernel is bound by the rate at which the vector-memory front end takes divergent lane loads
// (about one lane-instruction per clock and CU, whatever its width), so the fourth load that a 64-byte node needs for
// its two child references costs a quarter of the node bandwidth. Here the references ride in the low mantissa byte of
// the eight x / y planes: byte k of ref[0] is the low byte of n0xy[k], byte k of ref[1] the low byte of n1xy[k]. The
// planes are used as they are, reference byte included: pack_node() (bvh_build.h) rounds every plane outward far enough
// (<= 511 ulp, 6e-5 relative) that the box stays conservative whatever that byte holds. z planes are exact.
struct BvhNodePacked {
  float n0xy[4];
  float n1xy[4];
  float nz[4];
};
// The slot a packed node occupies in HBM. 48: nodes back to back (a node then straddles a 64-byte boundary every other
// time and a 128-byte line 3 times in 8). 64: one node per half line, 16 bytes of padding.
#ifndef STHIP_NODE_STRIDE
#define STHIP_NODE_STRIDE 48
#endif
#define BVH_NODE_BYTES ((unsigned)STHIP_NODE_STRIDE)
struct BvhNodeSlot {
  BvhNodePacked n;
#if STHIP_NODE_STRIDE > 48
  uint32_t pad[(STHIP_NODE_STRIDE - 48) / 4];
#endif
};
// The 4-wide node k_trace can walk instead ("wide_bvh"; bvh_build.h: build_wide_bvh collapses the binary tree into it): 64
// aligned bytes = four 16-byte loads per lane. The boxes of up to four children as 8-bit planes on a per-node grid:
// plane = origin[axis] + q * 2^exp[axis] (exp a signed byte), lower planes rounded down and upper planes up on that grid (exactly: the
// builder checks them in double), so a decoded box contains the child's box. An unused child slot (index >= exp[3])
// has its lower planes at 255 and its upper planes at 0 — the entry plane lies behind the exit plane on every axis, a miss
// unless the node is point-sized — and a copy of the first child's reference, so that even then nothing but a repeated
// visit can happen. References are the binary tree's, except that an inner
// reference indexes THIS array.
struct WideNode {
  float origin[3];
  uint8_t exp[4];    // exponents of the x, y, z plane step as signed bytes (-126 .. 127); [3] = number of children (not read by the kernel)
  uint8_t q[6][4];   // [lo.x, hi.x, lo.y, hi.y, lo.z, hi.z][child]
  uint32_t pad[2];
  uint32_t ref[4];
};
// The triangles of one leaf of the 4-wide tree as ONE record ("leaf_pairs"; bvh_build.h: build_leaf_pairs): 64 aligned bytes =
// four 16-byte loads in one round trip, where BvhTri takes three loads per triangle and a round trip each. A leaf's two
// triangles that share an edge have four vertices between them: A = (p0, p1, p2) is the leaf's first triangle in its own
// vertex order, B its second, also in its own order, as one of two fixed patterns over the four vertices (the triangle test's
// t, b1, b2 and edge signs depend on the order; shared vertices are bit-equal positions):
//   LEAF_PAIR_SINGLE  a one-triangle leaf: p3 = p0, id_b = 0xFFFFFFFF, B is never tested
//   LEAF_PAIR_FAN     B = (p0, p2, p3): the other half of a quad cut along p0 - p2
//   LEAF_PAIR_STRIP   B = (p1, p3, p2): the next triangle of a strip over the edge p1 - p2
//   LEAF_PAIR_SPLIT   a two-triangle leaf that fits neither pattern in either order: a one-triangle record of A here, and a
//                     LEAF_PAIR_SINGLE record of B in the next slot, which the lane visits in its next leaf phase
// The builder may swap the two triangles of a leaf (in BvhTri too: hits do not depend on their order) to reach a pattern.
// The record of the leaf whose first triangle is BvhTri f lies at index f, so a leaf reference — unchanged, the binary tree's —
// needs no second index; the slot behind the record of a two-triangle leaf is unused unless the leaf is split. When a tree
// has records every triangle leaf its wide nodes refer to has one. hit.leaf stays the BvhTri index (first for A, first + 1
// for B). The array costs 64 bytes per leaf triangle of device memory (51 MB on the 801 256 leaf triangles of the atrium).
// WRITERS of leaf-triangle positions, and what each does about the records:
//   api.hip install_tree        host build: writes BvhTri and the records together (build_leaf_pairs)
//   refit.hip k_refit_gather    new positions into BvhTri only — vertices that were bit-equal need not stay so; the records are
//   animate.hip k_animate         dropped before it runs (api.hip refit_resident_scene) and the wide form is collapsed again
//                                 from the binary tree
//   lbvh.hip / wide.hip         device build and device collapse: no records (api.hip clear_wide)
// READERS: k_trace<COUNT, false, BOUNDED, false, 3> (traverse.h: Traversal::pair_step) and nothing else.
#define LEAF_PAIR_SINGLE 0u
#define LEAF_PAIR_FAN 1u
#define LEAF_PAIR_STRIP 2u
#define LEAF_PAIR_SPLIT 3u
struct LeafPair {
  float p0[3];
  uint32_t id_a;   // BvhTri::id of A
  float p1[3];
  uint32_t id_b;   // ... of B; 0xFFFFFFFF (an id that never wins a tie and is never exposed) for LEAF_PAIR_SINGLE
  float p2[3];
  uint32_t first;  // the leaf's first BvhTri (= this record's index)
  float p3[3];
  uint32_t form;   // LEAF_PAIR_*
};
// The 8-wide compressed node ("wide_bvh" = 3; bvh_build.h: build_wide8_bvh): 80 bytes = five 16-byte loads per lane, after
// Ylitie, Karras, Laine, "Efficient Incoherent Ray Traversal on GPUs Through Compressed Wide BVHs" (HPG 2017). The boxes of
// up to eight children as 8-bit planes on the node's grid (as WideNode). No child references: the INNER children of a node
// are consecutive nodes of this array from child_base on, in slot order (child of slot s = child_base + popcount(imask &
// ((1 << s) - 1))); its LEAF children's items (triangles; top-level entries in a node of the top level) are consecutive
// from leaf_base on. So what a walk keeps of a visited node is a GROUP — a base and a bit mask — and its stack holds groups.
//   meta[s]: 0 = unused slot; inner child: 0x20 | (24 + s); leaf child: (unary item count: 1, 3 or 7) << 5 | first item
//   (relative to leaf_base, < 24). A hit child contributes (meta >> 5) << (meta & 31) to the 32-bit hit mask of the node:
//   items in bits 0..23, inner children in bits 24..31 — the latter at 24 + (s ^ octinv), octinv = 7 ^ (sign bits of the
//   ray direction), so that the highest set bit is the child to visit first: the builder puts the child lying toward the
//   (+x, +y, +z) corner of the node into slot 7, toward (-x, -y, -z) into slot 0, and so on.
// Slots are filled sparsely (by position); an unused slot also has entry planes behind its exit planes.
struct Wide8Node {
  float origin[3];
  uint8_t exp[3];       // signed exponents of the x, y, z plane step
  uint8_t imask;        // slots that hold inner children
  uint32_t child_base;  // index of the first inner child in this array
  uint32_t leaf_base;   // first item of the leaf children: a triangle index, or WIDE8_ENTRY_BIT | index into the entry table
  uint8_t meta[8];
  uint8_t q[6][8];      // [lo.x, hi.x, lo.y, hi.y, lo.z, hi.z][slot]
};
#define WIDE8_ENTRY_BIT 0x80000000u
#define WIDE8_MAX_ITEMS 24
#define BVH_NO_ALPHA 0xFFFFFFFFu  // DeviceBvh::inst_alpha entry of an instance whose material has no alpha mask
// uv of the three vertices of a leaf triangle, in leaf order next to BvhTri; only built for scenes with alpha masks
struct BvhTriUv {
  float uv[3][2];
};

// One entry of the top level: the merged world-space mesh (all instances whose transform is the identity,
// flattened into one BLAS), one transformed triangle instance, or one sphere instance (tested in place, no BLAS).
#define TLAS_ENTRY_TRANSFORMED 0u
#define TLAS_ENTRY_IDENTITY 1u
#define TLAS_ENTRY_SPHERE 2u
#define TLAS_ENTRY_VOLUME 3u  // root = index into DeviceBvh::volumes; tested in place by the instantiations that carry it
struct TlasEntry {
  float inv[12];      // gInstanceInverseTransforms[instance], row-major 3x4
  uint32_t root;      // index of the BLAS root (always an inner node); unused for a sphere
  uint32_t id_bits;   // OR-ed into BvhTri::id: 0 for the merged mesh, the instance index otherwise
  uint32_t identity;  // TLAS_ENTRY_*
  uint32_t pad;
  float center[3];    // object-space bounding sphere of the mesh: sizes the per-ray box padding
  float radius;       // ... or the radius of the sphere instance (InstanceData::radius, scene.h:43)
};

// The header of one NanoVDB float grid of gVolumes[], parsed on the host at upload (media.h reads the tree through it)
struct DeviceVolume {
  uint32_t first_word;  // the grid's first 32-bit word in DeviceVolumes::words
  uint32_t bytes;
  uint32_t root;        // byte address of the root node inside the grid
  uint32_t pad;
  int32_t bbox_min[3], bbox_max[3];
  float root_max, pad1;
  float matf[9], invmatf[9], vecf[3];
  float pad2[3];
};

// ---- what the upload lays out on the host (scene_prepare.cpp) and the kernels read as it is ----
// gImages (shading.h samples them): the mip chain of one image in image_texels / image_texels8
#ifndef STHIP_MAX_MIPS
#define STHIP_MAX_MIPS 16
#endif
struct DeviceImage {
  uint32_t offset[STHIP_MAX_MIPS];  // first texel of each level in image_texels (format 0) or in image_texels8 (format 1)
  uint16_t w[STHIP_MAX_MIPS], h[STHIP_MAX_MIPS];
  uint32_t levels;
  uint32_t format;  // sthip_image_format: STHIP_IMAGE_FORMAT_RGBA32F / STHIP_IMAGE_FORMAT_RGBA8_UNORM, uniform per image
  uint32_t pad[2];
};
// gImage1s, the alpha masks (traverse.h samples them): level 0 only
struct DeviceImage1 {
  uint32_t offset, w, h;  // offset: first texel in image1_texels (format 0) or in image1_texels8 (format 1)
  uint32_t format;        // sthip_image_format: STHIP_IMAGE_FORMAT_R32F / STHIP_IMAGE_FORMAT_R8_UNORM
};
// One emissive triangle instance: the box of its vertices in the space the traversal tests its triangles in (world space for an
// instance with identity transforms, the instance's object space otherwise) and a sphere around it that sizes the per-ray
// padding of the slab test exactly as the traversal's own boxes are padded (setup_space).
struct EmitterBounds {
  float lo[3];
  uint32_t instance;
  float hi[3];
  uint32_t identity;
  float sphere[4];
};
#define STHIP_MAX_EMITTER_BOUNDS 16u
// DisneyMaterial::Le() > 0 somewhere / can_eval() / is_specular() of an instance's untextured material, evaluated on the host with
// the device's arithmetic at upload (scene_prepare.cpp); KEEP: not a triangle instance, no statement made
#define INST_FLAG_EMITS 1u
#define INST_FLAG_CAN_EVAL 2u
#define INST_FLAG_SPECULAR 4u
#define INST_FLAG_KEEP 0x80u

#ifdef __cplusplus
static_assert(sizeof(BvhNode) == 64, "BvhNode");
static_assert(sizeof(BvhNodePacked) == 48, "BvhNodePacked");
static_assert(sizeof(BvhNodeSlot) == BVH_NODE_BYTES, "BvhNodeSlot");
static_assert(sizeof(BvhTri) == 48, "BvhTri");
static_assert(sizeof(BvhTriShade) == 64, "BvhTriShade");
static_assert(sizeof(WideNode) == 64, "WideNode");
static_assert(sizeof(Wide8Node) == 80, "Wide8Node");
static_assert(sizeof(LeafPair) == 64, "LeafPair");
static_assert(BVH_MAX_LEAF_TRIS <= 2, "a LeafPair record holds at most two triangles");
static_assert(sizeof(TlasEntry) == 80, "TlasEntry");
#endif
