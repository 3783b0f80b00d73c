/* sthip.h — C ABI of libstratum_hip.so: the MI355X path-tracing inner loop of Stratum.
 *
 * This library replaces exactly two things in the reference:
 *   - the Slang/HLSL ray-trace pipeline in src/Shaders (entry points
 *     sample_visibility, bdpt.hlsl:149-300, and trace_shadows, bdpt.hlsl:302-326,
 *     and everything they call), and
 *   - the Vulkan dispatch sequence that BDPT::render records for them
 *     (src/Node/BDPT.cpp:423-838; dispatch_over, src/Core/CommandBuffer.hpp:183-197),
 *     together with the driver-side acceleration structure it relies on
 *     (src/Core/AccelerationStructure.cpp:5-27, src/Node/Scene.cpp:435-459,614-629).
 * Everything above it (Node graph, Scene::update, loaders, GUI) stays as it is and
 * hands over the same arrays it binds to the shaders today; field names below are the
 * reflected binding names the reference uses ("gSceneParams.gVertices", ...,
 * BDPT.cpp:401-417,611-629; parameter blocks bdpt.hlsl:19-62).
 *
 * Conventions: plain pointers and sizes, no exceptions across the ABI; every call
 * returns 0 on success or a negative sthip_status, and sthip_last_error() returns a
 * description. A context is single-threaded; one context per GPU. There is no CPU
 * backend: without a HIP device sthip_create fails.
 */
#ifndef STHIP_H
#define STHIP_H

#include <stdint.h>
#include "sthip_wire.h"

#ifdef __cplusplus
extern "C" {
#endif

#define STHIP_ABI_VERSION 11

typedef struct sthip_ctx sthip_ctx;

enum sthip_status {
  STHIP_OK = 0,
  STHIP_ERR_INVALID_ARGUMENT = -1,
  STHIP_ERR_NO_DEVICE = -2,
  STHIP_ERR_HIP = -3,
  STHIP_ERR_UNSUPPORTED = -4, /* a flag / scene feature outside the built hot path */
  STHIP_ERR_NO_SCENE = -5
};

typedef struct sthip_image_desc {
  const float* pixels; /* width * height * 4 floats (gImage1s: width * height floats); bytes instead with an 8-bit format
                          of sthip_scene_upload_formats, see sthip_image_format */
  uint32_t width, height;
} sthip_image_desc;

/* ---- resident texel formats (sthip_scene_upload_formats) ----
 * Every texture the reference renders from is 8 bits per channel (Scene.cpp:178,229 create the material images as
 * R8G8B8A8Unorm, :182,233 the alpha masks as R8Unorm). An image may be handed over and kept resident in that form: a
 * quarter of the bytes on the host link, in HBM and per texel fetch. The format is chosen per image; format 0 is the
 * binary32 form sthip_scene_upload has always taken, stored and sampled exactly as before.
 *
 * Formats of gImages:  STHIP_IMAGE_FORMAT_RGBA32F (0): `pixels` points at width * height * 4 floats.
 *                      STHIP_IMAGE_FORMAT_RGBA8_UNORM (1): `pixels` points at width * height * 4 BYTES, row 0 first, R G B A.
 * Formats of gImage1s: STHIP_IMAGE_FORMAT_R32F (0): width * height floats.
 *                      STHIP_IMAGE_FORMAT_R8_UNORM (1): width * height BYTES.
 * Resident formats stay Unorm: the images the reference binds after material_convert are all Unorm, and a resident byte is
 * never passed through a transfer curve. The two images upstream binds undecoded — the sRGB emission image of an emissive
 * material and the RGB8 normal map — and every other format an asset holds (sRGB, one to three channels, 16-bit, BC1-BC5)
 * are decoded on the way in: sthip_texel_format and sthip_decode_texels below.
 *
 * Decode: a byte b is the binary32 quotient (float)b / 255.0f, correctly rounded (IEEE division; the build has no
 * fast-math and no contraction).
 * Mip chain of an RGBA8 image: the shape of the float chain — level k + 1 has max(1, dim / 2) texels per side, at most
 * STHIP_MAX_MIPS (16) levels, down to 1 x 1 — and each channel of texel (x, y) of level k + 1 is the integer
 *   (a + b + c + d + 2) >> 2
 * over the texels (min(2x, w - 1) | min(2x + 1, w - 1), min(2y, h - 1) | min(2y + 1, h - 1)) of level k, the four clamped
 * source texels of the float chain. Levels are stored as bytes; they are built on the device from the uploaded level 0
 * (one launch per level), so only level 0 crosses the host link. (An alpha mask has no chain: only level 0 is sampled.)
 * Filtering is unchanged: repeat addressing, bilinear taps, the trilinear blend between two levels, the same arithmetic
 * in the same order, applied to decoded texels.
 *
 * What follows for results: wherever only level 0 is read — without eRayCones (lod = 0), and in the alpha test — an 8-bit
 * image gives, bit for bit, what the float image pixels = bytes / 255.0f gives; and so at every level for an image whose
 * float chain ((a + b) + (c + d)) * 0.25f equals its decoded byte chain. Elsewhere the two chains differ by the rounding
 * of the integer mean (at most half a step of 1 / 255 per level).
 *
 * An 8-bit image bound as the environment map is refused by sthip_render and sthip_render_async with
 * STHIP_ERR_UNSUPPORTED and a message (an HDR environment in 8 bits is nobody's use case). */
#define STHIP_MAX_MIPS 16 /* levels of a mip chain at most, float or 8-bit */
enum sthip_image_format {
  STHIP_IMAGE_FORMAT_RGBA32F = 0,
  STHIP_IMAGE_FORMAT_RGBA8_UNORM = 1,
  STHIP_IMAGE_FORMAT_R32F = 0,
  STHIP_IMAGE_FORMAT_R8_UNORM = 1
};

typedef struct sthip_volume_desc {
  const void* data; /* the NanoVDB grid buffer */
  uint64_t bytes;
} sthip_volume_desc;

/* gSceneParams (bdpt.hlsl:19-35) as produced by Scene::update (Scene.cpp:299-684,
 * Scene.hpp:46-69). All pointers are host pointers, borrowed for the call and copied to HBM. */
typedef struct sthip_scene_desc {
  const sthip_PackedVertexData* gVertices; /* Scene.cpp:643-658 */
  uint32_t vertex_count;
  const void* gIndices; /* byte buffer, per-instance stride 2 or 4 (scene.h:139-161) */
  uint32_t indices_bytes;
  const sthip_InstanceData* gInstances; /* Scene.cpp:398-427 */
  uint32_t instance_count;
  const sthip_TransformData* gInstanceTransforms;
  const sthip_TransformData* gInstanceInverseTransforms;
  const sthip_TransformData* gInstanceMotionTransforms; /* may be NULL: identity */
  const void* gMaterialData; /* Material::store records, Material.hpp:32-38 */
  uint32_t material_bytes;
  const uint32_t* gLightInstances; /* Scene.cpp:406-409 */
  uint32_t light_count;
  /* Texture2D<float4> gImages[gImageCount] (bdpt.hlsl:33): what ImageValue::image_index refers to. RGBA32F,
   * row-major, row 0 first. The library builds the mip chain (2x2 box filter) and samples with repeat
   * addressing and trilinear filtering (the reference's gSamplerRepeat, BDPT.cpp:130-133, minus its 8x
   * anisotropy, which hardware-defined filtering cannot be restated). May be NULL / 0. */
  const struct sthip_image_desc* gImages;
  uint32_t image_count;
  /* StructuredBuffer<float> gDistributions (bdpt.hlsl:27): the concatenated distribution tables
   * MaterialResources::get_index(Buffer::View<float>) hands out offsets into (image_value.h:56-66, Scene.cpp:670-683);
   * here the four tables of the environment map (environment.h:17-22, built by dist2.h build_distributions).
   * May be NULL / 0. */
  const float* gDistributions;
  uint32_t distribution_count;
  /* Texture2D<float> gImage1s[] (bdpt.hlsl:34): what Material::alpha_mask refers to (MaterialRecord.alpha_mask_index,
   * Material.hpp:35). One float per texel (the reference stores R8Unorm coverage, Scene.cpp:182), row 0 first. With
   * eAlphaTest a triangle of a material that has a mask is hit only where the mask, sampled bilinearly with repeat
   * addressing at the hit's uv, is >= 0.75 (intersection.hlsli:117-131) — for closest-hit and shadow rays alike.
   * May be NULL / 0. */
  const struct sthip_image_desc* gImage1s;
  uint32_t image1_count;
  /* ByteAddressBuffer gVolumes[] (bdpt.hlsl:35): what InstanceData::volume_index (scene.h:46) and the Medium record's
   * density / albedo volume indices (Material.hpp:80-87) refer to. Each entry is one NanoVDB grid of type float exactly
   * as nanovdb::GridHandle holds it (format version 32.3, the NanoVDB the reference vendors). May be NULL / 0. */
  const struct sthip_volume_desc* gVolumes;
  uint32_t volume_count;
} sthip_scene_desc;

/* gFrameParams view arrays (bdpt.hlsl:37-43), filled by BDPT::render (BDPT.cpp:444-467).
 * gPrevViews / gPrevInverseViewTransforms may be NULL: static camera (previous = current). */
typedef struct sthip_frame_desc {
  const sthip_ViewData* gViews;
  const sthip_TransformData* gViewTransforms;
  const sthip_TransformData* gInverseViewTransforms;
  const sthip_ViewData* gPrevViews;
  const sthip_TransformData* gPrevInverseViewTransforms;
  uint32_t view_count;
  /* gViewMediumInstances (bdpt.hlsl:43, filled at BDPT.cpp:456-466): per view the volume instance the camera is inside
   * of, or 0xFFFF. May be NULL: every camera is outside every medium. */
  const uint32_t* gViewMediumInstances;
} sthip_frame_desc;

/* Output images/buffers of the two passes (bdpt.hlsl:44-49, BDPT.cpp:553-558).
 * gRadiance is required, the others may be NULL. With device_ptrs = 1 every non-NULL
 * pointer is a device pointer on the context's GPU (no copy; results are complete when
 * the call's stream work is complete, see sthip_set_stream).
 * Half colour precision (sthip_set_option "half_color_precision" = 1, the reference's mHalfColorPrecision,
 * BDPT.cpp:231,553-558): the three colour images gRadiance (both layouts), gAlbedo and gDebugImage (in and out) are
 * RGBA16F instead of RGBA32F — 8 bytes per pixel, four IEEE binary16 values in rgba order; the float* points at halves.
 * gVisibility, gDepth, gPrevUVs (RG32F upstream too) and gRayCount do not change. The arithmetic is the binary32 one;
 * a value is rounded to nearest even (det_f32tof16) only where it leaves the call: the radiance mean once, at its store;
 * the albedo once; the debug image at every seed (the seeds of a call are successive frames), so a call of N seeds
 * equals N chained calls of one. Hence radiance / albedo = RTNE(the binary32 call's arrays), bit for bit, and a 1-seed
 * call's debug image = RTNE(the binary32 call given the upcast half image). Upstream also rounds at each
 * read-modify-write of gRadiance / gDebugImage within a frame (trace_shadows, add_light_trace, debug `+=`); here the
 * running value stays binary32 between those statements. */
#define STHIP_LAYOUT_IMAGE 0u       /* gRadiance is the W x H image; pixels the shard does not own are zero */
#define STHIP_LAYOUT_SHARD_TILES 1u /* gRadiance holds only the shard's tiles, in slot order: sthip_shard_slot_count() float4 */
typedef struct sthip_outputs {
  uint32_t device_ptrs;
  uint32_t radiance_layout; /* STHIP_LAYOUT_*: the packed form is what ranks exchange (sthip_assemble_tiles) */
  float* gRadiance;                  /* RGBA32F (RGBA16F: half colour precision), W*H*4: rgb = mean over the seeds of this call, a = sample count */
  float* gAlbedo;                    /* RGBA32F (RGBA16F: half colour precision) */
  sthip_VisibilityInfo* gVisibility; /* W*H */
  sthip_DepthInfo* gDepth;           /* W*H */
  float* gPrevUVs;                   /* RG32F, W*H*2 */
  uint64_t* gRayCount;               /* [2]: all trace_ray calls / path (non-shadow) rays; intersection.hlsli:66, path.hlsli:1006 */
  /* BDPTDebugMode (bdpt.h:177-193; a specialisation constant of the reference's pipeline, BDPT.cpp:526-541) and the image it
   * feeds, RGBA32F W x H (bdpt.hlsl:45), with gDebugViewPathLength / gDebugLightPathLength of the push constants. gDebugImage
   * is IN / OUT as upstream's is (it persists from frame to frame): ePathLengthContribution and eViewTraceContribution start
   * every pixel's sample at (0,0,0,1), the other modes overwrite a pixel where a path reaches their statement or add to what it
   * holds; pixels outside every view are not touched. The seeds of a call are the reference's successive frames. 0 or a NULL
   * image = off (the image is then neither read nor written). Host or device pointer as the others (device_ptrs). */
  uint32_t debug_mode;
  float* gDebugImage;
} sthip_outputs;

enum {
  STHIP_DEBUG_NONE = 0,
  STHIP_DEBUG_ALBEDO,                     /* = m.albedo() of the first hit */
  STHIP_DEBUG_SPECULAR,                   /* = m.is_specular() */
  STHIP_DEBUG_EMISSION,                   /* = m.Le() */
  STHIP_DEBUG_SHADING_NORMAL,             /* = n * .5 + .5 (after the normal map) */
  STHIP_DEBUG_GEOMETRY_NORMAL,
  STHIP_DEBUG_DIR_OUT,                    /* = the last sampled direction * .5 + .5 */
  STHIP_DEBUG_PREV_UV,                    /* = |prev uv - uv| * extent */
  STHIP_DEBUG_ENVIRONMENT_SAMPLE_TEST,    /* += eight environment samples as spots around the view direction; nothing is traced */
  STHIP_DEBUG_ENVIRONMENT_SAMPLE_PDF,     /* .rgb = the environment's pdf of the view direction; nothing is traced */
  STHIP_DEBUG_RESERVOIR_WEIGHT,           /* += W of the NEE reservoir's sample where it is unoccluded (inline shadow rays only, as upstream) */
  STHIP_DEBUG_PATH_LENGTH_CONTRIBUTION,   /* the unweighted contributions of (gDebugViewPathLength, gDebugLightPathLength) */
  STHIP_DEBUG_LIGHT_TRACE_CONTRIBUTION,   /* light tracing's splats with weight 1 */
  STHIP_DEBUG_VIEW_TRACE_CONTRIBUTION,    /* += the unweighted emission view paths find; light tracing is not added to gRadiance */
  STHIP_DEBUG_MODE_COUNT
};

/* ---- lifetime ---- */
int sthip_abi_version(void);
int sthip_create(int device, sthip_ctx** out_ctx); /* replaces Device/pipeline creation, BDPT.cpp:35-41,151-187 */
void sthip_destroy(sthip_ctx* ctx);
const char* sthip_last_error(const sthip_ctx* ctx); /* ctx may be NULL: error of a failed sthip_create */

/* Stream the kernels are enqueued on (a hipStream_t; NULL = default stream). With host
 * output pointers sthip_render synchronises before returning; with device pointers it only
 * enqueues. */
int sthip_set_stream(sthip_ctx* ctx, void* hip_stream);

/* ---- scene: replaces BLAS/TLAS build + descriptor writes (Scene.cpp:429-509,614-629; BDPT.cpp:341-421) ----
 * Both scene calls first wait for the work already enqueued on the context's stream (frames of the previous scene that
 * were rendered with device output pointers), then replace the resident arrays: a caller never has to synchronise
 * before re-uploading.
 * The arguments are checked first, everything that can be decided without building the acceleration structure: a call
 * refused there (STHIP_ERR_INVALID_ARGUMENT: a NULL array, an index or address out of range, a bad image, a format that is
 * none; STHIP_ERR_UNSUPPORTED: 8-bit texels beyond 32-bit offsets) changes nothing but sthip_last_error — the previous scene
 * stays resident and renderable, with its rigs and everything kept for it. A failure after that (the builder refuses the
 * meshes, a HIP error) leaves NO scene resident. A scene wrong in one way gets the code and message it always got; of two
 * mistakes at once, one found by these checks is reported before one only the builder finds. */
int sthip_scene_upload(sthip_ctx* ctx, const sthip_scene_desc* scene);

/* sthip_scene_upload with a resident format per image (sthip_image_format above): image_formats has scene->image_count
 * entries for gImages, image1_formats scene->image1_count entries for gImage1s; a NULL array means all 0, and
 * sthip_scene_upload IS this call with both arrays NULL. An entry that is not a format of its array returns
 * STHIP_ERR_INVALID_ARGUMENT. The formats belong to the scene: the copy "keep_scene" keeps holds 8-bit images as bytes
 * with their formats, and everything built again from it (a moved instance of the merged mesh, a layout the refit does
 * not serve, the failure fallback) is built with them.
 *
 * sthip_scene_read_image: the stored texels of level `level` of gImages[image_index] in the image's resident format,
 * copied to host memory after the work on the stream has finished: w * h * 16 bytes (RGBA32F) or w * h * 4 bytes
 * (RGBA8) with w = max(1, width >> level), h = max(1, height >> level). out_bytes must be exactly that. It is how a
 * host (or a test) sees the mip chain. STHIP_ERR_INVALID_ARGUMENT: no scene, an index or a level out of range, a NULL
 * `out`, a wrong out_bytes. A library without the feature lacks the two symbols. */
int sthip_scene_upload_formats(sthip_ctx* ctx, const sthip_scene_desc* scene, const uint8_t* image_formats, const uint8_t* image1_formats);
int sthip_scene_read_image(sthip_ctx* ctx, uint32_t image_index, uint32_t level, void* out, uint64_t out_bytes);

/* Instances moved, nothing else changed (Scene::update with cached BLASes, Scene.cpp:435-459,614-629: only the TLAS is
 * rebuilt): new gInstanceTransforms / gInstanceInverseTransforms / gInstanceMotionTransforms (may be NULL: identity) for
 * the instance_count instances of the last sthip_scene_upload. The bottom levels stay in HBM, the top level is rebuilt
 * over the new world boxes. Instances whose transform was the identity at upload are part of one merged world-space
 * mesh: when one of THEM moves the resident tree cannot follow and the call builds the scene again, from the copy of the
 * arrays the context keeps since the upload ("keep_scene" = 1, the default) and the new transforms, with the configured
 * builder ("bvh_builder" = 1: ~10 ms per million triangles on the device) — sthip_stats::full_rebuilds counts these.
 * With "keep_scene" = 0 nothing is kept and such a call returns STHIP_ERR_UNSUPPORTED and changes nothing. */
int sthip_scene_update_transforms(sthip_ctx* ctx, const sthip_TransformData* gInstanceTransforms, const sthip_TransformData* gInstanceInverseTransforms,
                                  const sthip_TransformData* gInstanceMotionTransforms, uint32_t instance_count);

/* ---- instance transforms from host or device memory; the top level built on the host or on the device (top_level.hip) ----
 * sthip_scene_set_transforms is the descriptor form of the call above. With device_ptr = 0, top_level = 0, all three arrays
 * given and derive_motion = 0 it IS sthip_scene_update_transforms: the same results, refusals and kept state. Beyond that:
 *   device_ptr = 1     every non-NULL array is device memory, readable in the order of the context's stream. With the host
 *                      builder the matrices are copied back once and today's path is taken.
 *   inverse_transforms = NULL   the inverse is derived: the adjugate of the 3x3 block over its determinant, evaluated in
 *                      binary64 in this order — c00 = a11*a22 - a12*a21, c01 = a12*a20 - a10*a22, c02 = a10*a21 - a11*a20,
 *                      det = a00*c00 + a01*c01 + a02*c02; rows {c00, a02*a21 - a01*a22, a01*a12 - a02*a11} / det,
 *                      {c01, a00*a22 - a02*a20, a02*a10 - a00*a12} / det, {c02, a01*a20 - a00*a21, a00*a11 - a01*a10} / det,
 *                      every quotient its own IEEE division; translation 0.0 - (i0*tx + i1*ty + i2*tz) from the unrounded
 *                      binary64 quotients; every result rounded to binary32 once, at the store; unfused arithmetic. It is
 *                      transform_inverse of the Python host and of host/stratum_hip.hpp; an identity gives an identity.
 *   derive_motion = 1  (motion_transforms must be NULL) motion = tmul(resident transform before the call, new inverse as
 *                      binary32) in binary32, rows dotted left to right: ((a0*b0j + a1*b1j) + a2*b2j) (+ a3 for j = 3).
 *                      motion_transforms = NULL with derive_motion = 0: identity, as in the call above.
 *   top_level = 1      the top level is built on the device: entry boxes, scene centre and radius are the values the host
 *                      builder computes for the same matrices (sphere, volume and transformed-mesh cases, the 8 corners in
 *                      its order, rows dotted left to right and unfused, its two padding formulas, the merged mesh's kept
 *                      box), bit for bit except for the sign of a zero. The tree is a Karras radix tree over 16-bit-per-axis
 *                      Morton keys of the box centres with the entry index in the low 16 bits of the key (so equal codes are
 *                      ordered by entry index), fitted bottom-up: any valid binary tree is acceptable to the walks, frames do
 *                      not depend on its shape; same inputs give the same nodes. One entry gets a node with the leaf in both
 *                      slots; no entries or a lone identity entry keep the walk at the merged mesh without a top level.
 * Phase order: check, reserve, wait for the stream and the frames in flight, work beside the resident arrays, ONE small
 * read-back (flags, scene box, height), install. Refusals leave everything as it was:
 *   STHIP_ERR_INVALID_ARGUMENT  no desc, a struct_size that is not sizeof(sthip_transforms_desc), NULL transforms, derive_motion
 *                      together with a motion array, top_level > 1; a derived inverse whose determinant is 0 or not finite;
 *                      with the device builder an entry box that is not finite.
 *   STHIP_ERR_UNSUPPORTED  an instance_count that is not the resident one; a top level that is too deep or does not fit; an
 *                      instance of the merged mesh whose new transform or inverse is not the identity while "keep_scene" = 0.
 *                      With a kept scene that last case builds the scene again from it (info.rebuilt = 1, full_rebuilds++).
 * Kept first hits are dropped (the scene serial advances), as by the call above. After a device-pointer call or a derived
 * array the host's copies of the matrices (the kept scene, the entries' inverses) are older than the device's; the library
 * fetches them before their next reader. Layouts whose top level is made on the host from host nodes ("wide_bvh" = 3,
 * "treetop") read the new binary nodes back once.
 *
 * sthip_scene_read_transforms: the resident records [first, first + count) of the three arrays (any out pointer may be NULL).
 * sthip_scene_read_top_level: the entry boxes as the contract above defines them (6 floats per entry: lo, hi), the binary
 * top-level nodes — planes as the packed nodes hold them, so rounded outward; a child is a node index of this array or
 * 0x80000000 | entry — the root's index, and {centre.xyz, radius}. Without a top level node_count = 0 and root = 0xFFFFFFFF.
 * entry_boxes / nodes may be NULL (counts only); node_capacity smaller than the node count: STHIP_ERR_INVALID_ARGUMENT.
 * The entry boxes are not kept by either builder: when asked for them the call computes them again on the device from the
 * resident matrices and entries (the kernel of the device builder; it uses the context's top-level staging, nothing resident
 * changes). So they say what the contract gives for what is resident, whichever builder made the nodes.
 * A library without the feature lacks the three symbols.
 * Measured on an MI355X (profiles/r12/top_level.json; all instances moving, medians of 9 calls; the call above from host
 * arrays against this call from device pointers with derived arrays and the device builder): 1 000 instances 1.17 against
 * 0.55 ms, 8 192 instances 6.17 against 0.49 ms, 65 533 instances 21.8 against 1.55 ms (device_ms 0.45 / 0.42 / 1.47). The
 * trade-off: the forest's 1920 x 1080 frame takes 1.662 ms under the device-built tree against 1.633 ms under the host-built
 * one (+1.7 %, resolved); the two synthetic scenes show no difference. */
typedef struct sthip_transforms_desc {
  const sthip_TransformData* transforms;         /* instance_count records */
  const sthip_TransformData* inverse_transforms; /* NULL: derived by the library */
  const sthip_TransformData* motion_transforms;  /* NULL: identity, or derived (derive_motion) */
  uint32_t instance_count;
  uint32_t device_ptr;    /* 1: every non-NULL array is device memory */
  uint32_t top_level;     /* 0: host builder (binned SAH); 1: device builder */
  uint32_t derive_motion; /* 1 (motion_transforms must be NULL): motion = tmul(resident transform before the call, new inverse) */
} sthip_transforms_desc;
typedef struct sthip_transforms_info { /* optional out-parameter, may be NULL */
  float device_ms, total_ms;
  uint32_t top_level_nodes, top_level_depth; /* depth: an upper bound of the real height, the one the stack depth is made from */
  uint32_t rebuilt;                          /* 1: fell back to a rebuild from the kept scene (a merged instance moved) */
  uint32_t builder_used;                     /* 0 host, 1 device */
} sthip_transforms_info;
typedef struct sthip_top_node {
  float lo[3];
  uint32_t child0;
  float hi[3];
  uint32_t child1;
} sthip_top_node; /* lo / hi: the union of the two child boxes the node holds */
int sthip_scene_set_transforms(sthip_ctx* ctx, const sthip_transforms_desc* desc, uint32_t struct_size, sthip_transforms_info* info);
int sthip_scene_read_transforms(sthip_ctx* ctx, uint32_t first, uint32_t count, sthip_TransformData* transforms, sthip_TransformData* inverse_transforms, sthip_TransformData* motion_transforms);
int sthip_scene_read_top_level(sthip_ctx* ctx, float* entry_boxes, sthip_top_node* nodes, uint32_t node_capacity, uint32_t* entry_count, uint32_t* node_count, uint32_t* root, float center_radius[4]);

/* A mesh deformed, nothing else changed (the reference rebuilds the BLAS of a dirty mesh, Scene.cpp:345,435-459): new
 * contents for the records [first_vertex, first_vertex + vertex_count) of gVertices — position, normal and both texture
 * coordinates; the index buffer, instances, materials and transforms are those of the last sthip_scene_upload. The range
 * is copied into the resident gVertices (and into the copy "keep_scene" keeps, so a later rebuild sees the deformed mesh);
 * then, on the device, every leaf triangle is gathered again through the index triple it came from, the shading records
 * beside the triangles are made again, and the boxes of the bottom levels are refitted bottom-up in place, one launch per
 * height of the tree; the top level, the entries' bounding spheres, the scene bounds, the emitter bounds of
 * "answer_last_rays" and the 4-wide form follow. The trees keep their shape: closest hit is the minimum over all triangles
 * (ties by id), so the frame is the one a fresh upload of the deformed scene gives, bit for bit, whatever the deformation
 * did to the quality of the tree. sah_cost / sah_cost_at_build says what it did: that ratio is the host's signal to upload
 * again (the walk slows down as it grows). Measured on the 1M-triangle atrium (profiles/r06/refit.json): 1.69 ms for the
 * call with all 408 970 vertices replaced (0.72 ms of it on the stream), 0.134 of the 12.57 ms the re-upload with the device
 * builder takes in the same run; the first call on a tree also makes the schedule, 8.2 ms; a sine displacement of 0.15 m
 * raises the cost ratio to 1.11 and the frame time to 1.03 of a freshly built tree's, one of 1 m to 1.77 and 1.15. Waits for the stream and completes the frames in flight first, as
 * sthip_scene_update_transforms does; kept reservoir grids ("reuse_grids_persist") are dropped, as at an upload.
 * Layouts the refit does not serve — "embed_leaves", "treetop", the 8-wide form of "wide_bvh" = 3 — are built again from
 * the kept scene instead (rebuilt = 1, counted in sthip_stats::full_rebuilds); with "keep_scene" = 0 the call then returns
 * STHIP_ERR_UNSUPPORTED and changes nothing. STHIP_ERR_INVALID_ARGUMENT: no scene, a NULL pointer, a range past the
 * uploaded vertex_count. Everything that can be refused or can run out of memory is checked or allocated before the
 * resident scene is touched, and a call that fails there leaves it as it was. Should a step fail after the vertices have
 * gone up (a HIP error, or a top level over the new boxes that is too deep or too large for what is resident), the scene is
 * never left with new triangles under an old top level: with a kept scene it is built again from it (rebuilt = 1); with
 * "keep_scene" = 0 the call returns the error and NO scene is resident afterwards, as after a failed sthip_scene_upload:
 * upload again. A library without the feature lacks the symbol. */
typedef struct sthip_refit_info { /* optional out-parameter, may be NULL */
  float device_ms;                /* stream time of gather + refit + derived forms (HIP events) */
  float total_ms;                 /* wall time of the call */
  float sah_cost;                 /* SAH cost of the bottom levels after the refit, same formula as sah_cost_at_build */
  float sah_cost_at_build;        /* the same cost of the tree as it was built, before any refit */
  uint32_t rebuilt;               /* 1: the call fell back to a full rebuild from the kept scene */
  uint32_t pad;
} sthip_refit_info;
int sthip_scene_update_vertices(sthip_ctx* ctx, const sthip_PackedVertexData* vertices, uint32_t first_vertex, uint32_t vertex_count, sthip_refit_info* info);

/* ---- rigs: a mesh animated on the device (kernels/anim.hlsl: `blend` :53-86, `skin` :27-51; no upstream host calls them) ----
 * sthip_scene_update_vertices needs the host to compute every deformed vertex and to send it up on each frame. Almost every
 * moving mesh is a rig: a rest pose, a few blend targets, four bone weights per vertex. With the calls below the rig stays
 * resident and a frame sends only its pose: four blend factors and bone_count matrices per rig. One kernel (animate.hip)
 * writes the rig's records of gVertices on the device; the gather, the refit, the top level and everything else
 * sthip_scene_update_vertices derives follow unchanged, so the frame is the one a fresh upload of the posed vertices gives,
 * bit for bit.
 *
 * The arithmetic is part of the contract (sthip_detmath.h: binary32, no contraction, left to right). Per vertex, rest record r:
 *   blend, only if blend_target_count > 0 (anim.hlsl:59-81):
 *     f = fmaxf(0, 1 - (((|b0| + |b1|) + |b2|) + |b3|));  p = f * r.position;  for k = 0 .. count - 1: p = p + bk * Tk.position;
 *     n the same from the normals, then n = normalize3(n) (1 / sqrt of the dot product, times each component). Without targets
 *     p and n are bit copies of the rest.
 *   skin, only if bone_count > 0 (anim.hlsl:31-45):
 *     M = +0;  for j = 0 .. 3: M = M + bones[indices[j]] * weights[j], elementwise;
 *     p' = M[r][0] * p.x + M[r][1] * p.y + M[r][2] * p.z + M[r][3];  n' the 3x3 part the same way; not renormalised (as upstream).
 *   u and v are bit copies of the rest. Upstream's tangent has no field in PackedVertexData and is not carried.
 *
 * sthip_scene_set_rigs: `rigs` and everything they point to are host arrays, copied during the call. Validated on the host:
 * STHIP_ERR_INVALID_ARGUMENT with a message, and nothing changes (rigs set before stay), when no scene is resident, a range
 * runs past the uploaded vertex_count, two ranges overlap, blend_target_count > 4 or bone_count > 1024, a pointer the counts
 * require is NULL (`weights` is NULL if and only if bone_count == 0), or some indices[k] >= bone_count. Then the REST POSE of
 * each rig is taken on the device: a copy of the records of its range as they are resident at this moment, whatever the last
 * upload, sthip_scene_update_vertices or sthip_scene_animate left there; targets and weights go up once. A later
 * sthip_scene_update_vertices over a rigged range changes the resident records until the next sthip_scene_animate but does
 * NOT change the rest pose: set the rigs again for that. rig_count = 0 drops all rigs; so does every sthip_scene_upload.
 *
 * sthip_scene_animate: pose_count must be the rig_count of the last sthip_scene_set_rigs, poses[i] belongs to rigs[i].
 * Refused on the host (STHIP_ERR_INVALID_ARGUMENT, nothing changes): no scene, no rigs, a wrong pose_count, `bones` NULL for a
 * rig with bones, a factor of a present target or a bone entry that is not finite. Then it does what
 * sthip_scene_update_vertices does with the upload replaced by the kernel: waits for the stream and completes the frames in
 * flight, sends the bones (the only host-to-device traffic of the call), launches k_animate once per rig, gathers, refits
 * and installs the new top level. sthip_refit_info as for the vertex call; device_ms includes k_animate.
 * Measured on the 1M-triangle atrium (profiles/r07/animate.json, medians of 9 calls, device-built tree): a rig over all
 * 408 970 vertices with 4 targets and 64 bones, 0.86 ms for the call (0.73 ms of it on the stream, k_animate included; 3 KB go
 * up) against 1.32 ms for sthip_scene_update_vertices with the same vertices in the same process (0.71 ms on the stream; 13 MB
 * go up); a rig over one instance's mesh (5 440 vertices) 0.83 ms against 0.84 ms.
 * The copy of the scene "keep_scene" keeps is NOT updated per call (that would bring the transfer back in the other
 * direction): its rigged ranges are marked stale and read back from the device immediately before anything is built again
 * from the kept scene — the rebuild inside sthip_scene_update_transforms when a merged instance moved, the failure fallback,
 * and the layouts the refit does not serve ("embed_leaves", "treetop", "wide_bvh" = 3), for which this call runs the kernel,
 * reads the ranges back and builds the scene again (rebuilt = 1). A sthip_scene_update_vertices over records of a stale range
 * makes those records current again. Failures follow the vertex call's rules: everything that can be refused or can run out
 * of memory happens before gVertices is touched; after that a failure ends in a rebuild from the kept scene, or with
 * "keep_scene" = 0 in no resident scene (layouts the refit serves) — layouts it does not serve return STHIP_ERR_UNSUPPORTED
 * with "keep_scene" = 0 and change nothing.
 *
 * sthip_scene_read_vertices: the resident records [first_vertex, first_vertex + vertex_count) of gVertices, copied to host
 * memory after the work on the stream has finished (what a host that wants the posed mesh back calls; tests).
 * A library without the feature lacks the three symbols. */
typedef struct sthip_rig_desc {
  uint32_t first_vertex, vertex_count;            /* the records of gVertices this rig drives */
  uint32_t blend_target_count;                    /* 0..4 */
  uint32_t bone_count;                            /* 0: no skinning; at most 1024 */
  const sthip_PackedVertexData* blend_targets[4]; /* vertex_count records each; position and normal are read, u / v ignored */
  const sthip_VertexWeight* weights;              /* vertex_count records, or NULL iff bone_count == 0 */
} sthip_rig_desc;
typedef struct sthip_rig_pose {
  float blend_factors[4];           /* factors of absent targets are taken as 0 */
  const sthip_TransformData* bones; /* bone_count matrices (row-major 3x4), NULL iff the rig has no bones */
} sthip_rig_pose;
int sthip_scene_set_rigs(sthip_ctx* ctx, const sthip_rig_desc* rigs, uint32_t rig_count);
int sthip_scene_animate(sthip_ctx* ctx, const sthip_rig_pose* poses, uint32_t pose_count, sthip_refit_info* info);
int sthip_scene_read_vertices(sthip_ctx* ctx, uint32_t first_vertex, uint32_t vertex_count, sthip_PackedVertexData* out);

/* ---- vertices from streams: a deformed mesh whose positions are already on the device (kernels/copy_vertices.hlsl) ----
 * sthip_scene_update_vertices takes finished records from host memory. A simulation that leaves positions on the device would
 * have to copy them back, make normals on the host, interleave records and send 32 B per vertex up again. This call takes the
 * strided position / normal / texcoord streams as they are — device memory (device_ptr = 1: read in the order of the context's
 * stream) or host memory (device_ptr = 0: the spans of the streams are copied into a staging buffer on the stream, then the same
 * kernels run) — packs them into the resident gVertices and, on request, makes the shading normals of the range again from
 * the moved positions. Everything after the write of gVertices is the chain of sthip_scene_update_vertices, unchanged: the
 * frames in flight are completed first, then gather, shading records, refit, top level, emitter bounds, the wide form; kept
 * reservoir grids are dropped. sthip_refit_info as for the vertex call; device_ms includes the new kernels.
 *
 * PACK CONTRACT (k_pack_vertices, vertex_streams.hip; PackedVertexData::set, copy_vertices.hlsl:29-37, scene.h:81-94):
 *   record first_vertex + i becomes {positions[i], u, normals[i], v} with (u, v) = texcoords[i], all as bit copies. The fields
 *   of an absent (NULL) stream keep their resident bits. Records outside the range are not written. Only 4-byte alignment is
 *   assumed of the streams; element i of a stream lies `stride` bytes behind element i - 1.
 *
 * NORMAL CONTRACT (recompute_normals = 1; k_face_vectors, k_vertex_normals). Arithmetic is binary32 and unfused, in the order
 * written (sthip_detmath.h):
 *   meshes:  the distinct tuples (indices_byte_offset, first_vertex, index_stride, prim_count) of the scene's triangle
 *            instances, in ascending order of that tuple; instances that share a tuple count once; spheres and volumes have none.
 *   face vectors:  for triangle t of mesh m the three indices are read as the refit reads them (zero-extended 16- or 32-bit,
 *            plus first_vertex); p0, p1, p2 are the resident positions after this call's write; e1 = p1 - p0, e2 = p2 - p0,
 *            g = (e1.y*e2.z - e1.z*e2.y, e1.z*e2.x - e1.x*e2.z, e1.x*e2.y - e1.y*e2.x), every product rounded before the
 *            subtraction (an area-weighted face normal, not normalised).
 *   sum and normalise:  for a vertex v of the range, s = +0; for every corner (m, t, c) whose absolute index is v, in
 *            ascending (m, t, c): s = s + g(m, t); d = (s.x*s.x + s.y*s.y) + s.z*s.z; if d > 0 and d < inf the normal becomes
 *            s * (1.0f / sqrtf(d)) (normalize3, as k_animate uses it), otherwise the resident normal stays.
 *   the resident normal therefore stays for a vertex no triangle names, a vertex whose face vectors sum to zero (all of its
 *            faces degenerate, or faces that cancel) and a NaN (or an overflow) in the sum.
 *   neighbours outside the range contribute their resident positions and are not rewritten themselves: a caller that moves
 *            a whole mesh passes the whole mesh.
 * The sum is made store-then-sum: every face vector goes to a slot of a scratch array, then one lane per vertex adds its
 * row of an adjacency in the contract's order. No float atomics decide anything, so the same positions give the same bytes.
 * The adjacency is made once per uploaded topology, at the first call that asks for normals, and dropped at every upload.
 *
 * Refused with STHIP_ERR_INVALID_ARGUMENT, a message that names the field, and nothing changed: no scene resident, a
 * struct_size below sizeof(sthip_vertex_streams), a NULL `positions`, a range past the uploaded vertex_count, a pointer or
 * stride of a present stream that is not a multiple of 4, a stride below the element size (12 / 12 / 8), `normals` together
 * with recompute_normals. vertex_count = 0 is a valid no-op (STHIP_OK). Failure rules are the vertex call's: everything that
 * can be refused or can run out of memory happens before gVertices is touched; afterwards a failure ends in a rebuild from
 * the kept scene, or with "keep_scene" = 0 in no resident scene. For the layouts the refit does not serve ("embed_leaves",
 * "treetop", "wide_bvh" = 3) the call runs the kernels, reads the range back into the kept scene and builds the scene again
 * (rebuilt = 1); with "keep_scene" = 0 it returns STHIP_ERR_UNSUPPORTED and changes nothing. The copy "keep_scene" keeps is
 * not written per call: the range is marked stale and fetched immediately before anything is built from the kept scene; a
 * later sthip_scene_update_vertices over part of the range makes that part current. Over a rigged range the call behaves as
 * sthip_scene_update_vertices does: the resident records change until the next sthip_scene_animate, the rest pose does not.
 * Measured on the 1M-triangle atrium (profiles/r15/vertices.json, medians of 9 calls, device-built tree, the forms alternating
 * in one process), all 408 970 vertices: 0.85 ms for the call from device streams with positions, normals and uvs and 0.88 ms
 * with positions only and recompute_normals, against 1.59 ms for sthip_scene_update_vertices with the same vertices sent up
 * (0.72 / 0.75 / 0.73 ms of them on the stream); the first call on a topology also makes the adjacency, 7.5 ms; one instance's
 * mesh (5 440 vertices): 0.83 / 0.85 against 0.84 ms. The kernels alone: k_pack_vertices 0.018 ms, k_face_vectors 0.014 ms,
 * k_vertex_normals 0.014 ms.
 * Measurement only: with the environment variable STHIP_VERTEX_TIMES=<file> (read once per process) every call appends one
 * JSON line to the file with the HIP-event time of each of its kernels (k_pack_vertices_ms, k_face_vectors_ms,
 * k_vertex_normals_ms; 0 for one that did not run) and waits for the stream behind them. Without the variable the call makes
 * no extra event and touches no file.
 * The ABI is additive (STHIP_ABI_VERSION stays 11): a library without the feature lacks the symbol. */
typedef struct sthip_vertex_streams {
  uint32_t struct_size;
  uint32_t first_vertex, vertex_count; /* records of gVertices that are written */
  uint32_t device_ptr;                 /* 1: the three streams are device memory, readable in the order of the context's stream */
  uint32_t recompute_normals;          /* 1: normals of the range are made on the device (contract above); `normals` must be NULL */
  uint32_t position_stride, normal_stride, texcoord_stride; /* bytes between elements */
  const void* positions;               /* float3 per vertex, required */
  const void* normals;                 /* float3 per vertex, or NULL: normals stay (or are recomputed) */
  const void* texcoords;               /* float2 per vertex (u, v), or NULL: u and v of the resident records stay */
} sthip_vertex_streams;
int sthip_scene_set_vertices(sthip_ctx* ctx, const sthip_vertex_streams* streams, sthip_refit_info* info);

/* ---- material conversion: where the images of a material come from (Scene.cpp:123-256 -> kernels/material_convert.hlsl) ----
 * The library renders from three R8G8B8A8Unorm images per material (DisneyMaterialData, disney_data.h) and one R8Unorm alpha
 * mask. Upstream makes them on the device from what an asset holds: Scene::make_metallic_roughness_material (glTF: base colour
 * + metallic/roughness) dispatches from_gltf_pbr (hlsl:46-76), Scene::make_diffuse_specular_material (Mitsuba / OBJ: diffuse +
 * specular + shininess) from_diffuse_specular (:78-108), Scene::alpha_to_roughness and Scene::shininess_to_roughness the two
 * one-channel kernels (:28-35, :37-44). sthip_convert_material is those four kernels; `kind` chooses one.
 *
 * Images are linear arrays of width * height texels, row 0 first. Sources: gDiffuse, gSpecular, gTransmittance — four
 * channels, STHIP_IMAGE_FORMAT_RGBA32F or _RGBA8_UNORM, a format byte each; gRoughness (DIFFUSE_SPECULAR) and gInput (the two
 * roughness kinds) — one channel, _R32F or _R8_UNORM. Every source format byte also takes a sthip_texel_format from 16 up (the
 * asset's own format, decoded in the kernel: see "source texel formats" below; 2 .. 15 are no format). A NULL source is
 * upstream's gUseX = false. A byte decodes as (float)b / 255.0f. Outputs: gOutput[3], the three DisneyMaterialData vectors per texel (data[0] = base colour rgb, emission;
 * data[1] = metallic, roughness, anisotropic, subsurface; data[2] = clearcoat, clearcoat gloss, transmission, eta);
 * gOutputAlphaMask, one channel, written only when gDiffuse is given; gOutputMinAlpha, one uint32_t, set to 0xFFFFFFFF by the
 * call itself and then reduced; gRoughnessRW (one channel) for the roughness kinds. output_format 1: bytes (RGBA8 / R8, what
 * upstream stores), 0: the unquantised binary32 values (RGBA32F / R32F).
 * device_ptrs as in the calls after the path: host form — the sources are staged, the outputs copied back, and the call
 * returns synchronised; device form — the clear of gOutputMinAlpha and one kernel are only enqueued on the context's stream,
 * nothing is allocated or waited for, and gOutputMinAlpha is a device pointer too. Device images are naturally aligned (an
 * RGBA8 image to 4 bytes, RGBA32F to 16, R32F to 4); all-8-bit images aligned to 16 bytes (one-channel ones to 4) take the
 * wide path: four texels per lane.
 *
 * THE ARITHMETIC CONTRACT. Binary32, unfused, in the source order of the shader; only IEEE + - * / and sqrtf, all correctly
 * rounded, so no det_* function is involved.
 *   luminance(c) = (c.x * 0.2126f + c.y * 0.7152f) + c.z * 0.0722f
 *   saturate(a)  = a > 0 ? (a < 1 ? a : 1) : 0, so a NaN gives 0.
 *   GLTF_PBR          base = gDiffuse.rgb, or 1 without gDiffuse; metallic = gSpecular.b, roughness = gSpecular.g, both 1 without
 *                     gSpecular; transmission = saturate(luminance(gTransmittance.rgb) / (l > 0 ? l : 1)) with l = luminance(base),
 *                     0 without gTransmittance. Every other channel (emission, anisotropic, subsurface, clearcoat, clearcoat
 *                     gloss, eta) is 1, as upstream's m.data[i] = 1.
 *   DIFFUSE_SPECULAR  d, s, t = the rgb of gDiffuse, gSpecular, gTransmittance, 0 where absent; ld, ls, lt their luminances;
 *                     den = (ls + ld) + lt; base = ((d * ld + s * ls) + t * lt) / den per channel; metallic = saturate(ls / den)
 *                     only with gSpecular, roughness = gRoughness only with gRoughness, transmission = saturate(lt / den) only
 *                     with gTransmittance; otherwise those channels stay 1, as all the others. 0 / 0 is a NaN and is kept in
 *                     the float form.
 *   ALPHA_TO_ROUGHNESS     saturate(sqrtf(x));  SHININESS_TO_ROUGHNESS  saturate(sqrtf(2 / (x + 2)))
 *   quantisation (output_format 1)  byte = (uint32_t)(saturate(v) * 255.0f + 0.5f): two operations and a truncation; a NaN
 *                     gives 0. Consequence: a byte that only passes through — GLTF base colour, metallic, roughness,
 *                     gRoughness, the alpha mask — comes out as the byte that went in (it holds for all 256 bytes).
 *   alpha             the mask receives gDiffuse.a, quantised as above or as it is. For texels with a < 1 (false for a NaN)
 *                     min_alpha = min(min_alpha, (uint32_t)(saturate(a) * 4294967296.0f)): upstream's 0xFFFFFFFF becomes 2^32
 *                     as a float, and the scaling is exact. The payload and sign of a NaN are not part of the contract.
 * Differences from upstream, stated: all given sources must have the extent width x height (upstream reads the others at the
 * first image's coordinates and relies on robust buffer access); the roughness result has output_format, not the input's.
 * Refused with STHIP_ERR_INVALID_ARGUMENT, the message naming the field: an unknown kind; an empty extent or one of more than
 * 2^30 texels; an output_format or the format byte of a given source that is none; no source at all for the two material
 * kinds; a NULL gInput / gRoughnessRW for the roughness kinds; a NULL gOutput[k] or gOutputMinAlpha; a NULL gOutputAlphaMask
 * although gDiffuse is given; with device_ptrs an image that is not naturally aligned. Fields a kind does not use are ignored.
 * A library without the feature lacks the symbol. */
enum {
  STHIP_CONVERT_GLTF_PBR = 0,
  STHIP_CONVERT_DIFFUSE_SPECULAR = 1,
  STHIP_CONVERT_ALPHA_TO_ROUGHNESS = 2,
  STHIP_CONVERT_SHININESS_TO_ROUGHNESS = 3,
  STHIP_CONVERT_KIND_COUNT
};
typedef struct sthip_convert_material_desc {
  uint32_t kind; /* STHIP_CONVERT_* */
  uint32_t width, height;
  uint32_t device_ptrs;
  uint32_t output_format; /* sthip_image_format of every output */
  uint8_t diffuse_format, specular_format, transmittance_format, roughness_format; /* sthip_image_format per source */
  uint8_t input_format;
  uint8_t pad_[7];
  const void* gDiffuse; /* also the base colour; rgba */
  const void* gSpecular; /* GLTF_PBR: the metallic/roughness image (b, g) */
  const void* gTransmittance;
  const void* gRoughness; /* one channel; DIFFUSE_SPECULAR */
  const void* gInput;     /* one channel; the roughness kinds */
  void* gOutput[3];
  void* gOutputAlphaMask;    /* one channel */
  uint32_t* gOutputMinAlpha; /* one word */
  void* gRoughnessRW;        /* one channel; the roughness kinds */
} sthip_convert_material_desc;
int sthip_convert_material(sthip_ctx* ctx, const sthip_convert_material_desc* desc);

/* ---- source texel formats: what an asset holds, decoded on the way in (load_gltf.cpp:42-56, Image.cpp:22-40,107-121) ----
 * Upstream's conversion shaders read Texture2D<float4>: the texture unit decodes the loader's format before the shader sees
 * a texel. A sthip_texel_format names such a format; sthip_decode_texels is that decode as a device stage, and the format
 * bytes of sthip_convert_material take the same values (the decode then happens in its kernels, no image in between).
 * Nothing resident changes: the renderer keeps RGBA32F / RGBA8_UNORM / R32F / R8_UNORM images, and a transfer curve is
 * applied only here, on the way in.
 *
 * VALUES. 0 and 1 keep their meaning (sthip_image_format: RGBA32F and RGBA8_UNORM, or R32F and R8_UNORM where the source has
 * one channel; in sthip_decode_texels they are the four-channel forms). 2 .. 15 stay no format. From 16 up:
 *   linear formats   16 + 4 * class + (channels - 1), class 0 unorm8, 1 sRGB8, 2 unorm16 (little-endian), 3 binary32
 *   block formats    32 .. 39
 *   48 .. 79         formats the loaders' table knows but no material path gives a meaning: named, refused with
 *                    STHIP_ERR_UNSUPPORTED and a message that names the format: snorm, integer and 64-bit formats, BC4 / BC5
 *                    snorm, BC6H, BC7.
 * Any other value is no format (STHIP_ERR_INVALID_ARGUMENT).
 *
 * LAYOUT. A linear image is width * height texels, tightly packed, row 0 first, the channels of a texel in the order R G B A.
 * A block image is ceil(width / 4) * ceil(height / 4) blocks, row-major, 8 bytes each (BC1, BC4) or 16 (BC2, BC3, BC5);
 * texel (x, y) lies in block (x / 4, y / 4) as its texel t = 4 * (y % 4) + (x % 4). Texels of a block beyond the extent are
 * never read as texels. Flipping and file parsing are the caller's: the API takes texels, not files.
 *
 * DECODE, to four binary32 channels. Absent channels: G = B = 0, A = 1. Every value is a real number rounded once by one
 * IEEE operation.
 *   unorm8    (float)b / 255.0f                         unorm16   (float)v / 65535.0f, v = lo | hi << 8
 *   binary32  the value as it is
 *   colour block (8 bytes: BC1, and bytes 8 .. 15 of BC2 and BC3)
 *             c0 = byte0 | byte1 << 8, c1 = byte2 | byte3 << 8, endpoints RGB565: red = c >> 11, green = (c >> 5) & 63,
 *             blue = c & 31. bits = byte4 | byte5 << 8 | byte6 << 16 | byte7 << 24; the index of texel t is
 *             (bits >> 2t) & 3. With e0, e1 the INTEGER endpoint values of a channel:
 *               index 0: (float)e0 / 31.0f  (63.0f for green)        index 1: (float)e1 / 31.0f  (63.0f)
 *               four-colour rule (BC1 with c0 > c1 as integers; BC2 and BC3 always):
 *                 index 2: (float)(2 * e0 + e1) / 93.0f (189.0f)     index 3: (float)(e0 + 2 * e1) / 93.0f (189.0f)
 *               three-colour rule (BC1 with c0 <= c1):
 *                 index 2: (float)(e0 + e1) / 62.0f (126.0f)         index 3: 0, 0, 0
 *             BC1_RGB: alpha is 1 for every index (the reference never asks for BC1 alpha).
 *   BC2 alpha (bytes 0 .. 7): the nibble of texel t is (byte[t / 2] >> 4 * (t % 2)) & 15; alpha = (float)a4 / 15.0f.
 *   RGTC block (8 bytes: BC4; bytes 0 .. 7 of BC3, its alpha; bytes 0 .. 7 of BC5 for R and bytes 8 .. 15 for G)
 *             r0 = byte0, r1 = byte1; bits = byte2 | byte3 << 8 | ... | byte7 << 40 (48 bits in bytes 2 .. 7); the index of
 *             texel t is (bits >> 3t) & 7.
 *               index 0: (float)r0 / 255.0f     index 1: (float)r1 / 255.0f
 *               r0 > r1:   index i = 2 .. 7: (float)((8 - i) * r0 + (i - 1) * r1) / 1785.0f
 *               r0 <= r1:  index i = 2 .. 5: (float)((6 - i) * r0 + (i - 1) * r1) / 1275.0f; index 6: 0; index 7: 1
 *             BC4: R, with G = B = 0, A = 1. BC5: R and G, B = 0, A = 1. BC3: RGB from its colour block, A from its RGTC block.
 *   sRGB      on R, G, B only (alpha is linear), applied to the binary32 value c of the rules above:
 *               c <= 0.04045f ? c / 12.92f : det_powf((c + 0.055f) / 1.055f, 2.4f)
 *             all binary32, unfused, det_powf of sthip_detmath.h. (A kernel may serve bytes from a 256-entry table made with
 *             this function; the table is no part of the contract.)
 * These are the ratios the Khronos Data Format Specification gives for S3TC and RGTC.
 *
 * sthip_decode_texels. Source: a format, a pointer, width and height. Destination: one of the library's four forms —
 * dst_channels 4: RGBA32F (dst_format 0) or RGBA8_UNORM (1); dst_channels 1: R32F (0) or R8_UNORM (1) of the channel
 * `channel` (0 .. 3) of the decoded texel. An 8-bit destination is quantised as in sthip_convert_material:
 * byte = (uint32_t)(saturate(v) * 255.0f + 0.5f). Consequence: a unorm8 source of any channel count into an 8-bit destination
 * gives the source bytes back, for all 256 values.
 * device_ptrs as in sthip_convert_material: host form — the source is staged, the destination copied back, the call returns
 * synchronised; device form — one kernel is enqueued on the context's stream, nothing is allocated or waited for. A device
 * pointer is naturally aligned: a block image to the size of its block (8 or 16 bytes), a linear image to the size of one
 * component (1, 2 or 4), the destination to its texel (16, 4, 4, 1). Linear 8-bit sources aligned to 4 bytes with a destination
 * aligned to 16 (R8: 4) go four texels per lane.
 * Refused with STHIP_ERR_INVALID_ARGUMENT, the message naming the field: an empty extent (width, height) or one of more than
 * 2^30 texels (width x height); src_format that is none; dst_format above 1; dst_channels other than 1 or 4; channel above 3;
 * a NULL src or dst; a device pointer that is not naturally aligned. A refused call writes nothing.
 * In sthip_convert_material every source format byte and input_format take these values; a one-channel source (gRoughness,
 * gInput) given in a multi-channel format takes channel 0, as a Texture2D<float> read does; the alignment of a device source
 * is the one above; all given sources still have the extent width x height. What every glTF file gives — gDiffuse
 * RGBA8_SRGB, the other sources format 1, 8-bit outputs — takes the all-8-bit kernel where gDiffuse is aligned as an RGBA8_UNORM
 * image is (16 bytes: four texels per lane); every other mix of formats goes one texel per lane. The results do not depend on
 * the path.
 * A library without the feature lacks the symbol sthip_decode_texels. */
enum sthip_texel_format {
  STHIP_TEXEL_RGBA32F = 0, /* = STHIP_IMAGE_FORMAT_RGBA32F */
  STHIP_TEXEL_RGBA8_UNORM = 1, /* = STHIP_IMAGE_FORMAT_RGBA8_UNORM */
  STHIP_TEXEL_FIRST = 16,
  STHIP_TEXEL_R8_UNORM = 16,
  STHIP_TEXEL_RG8_UNORM = 17,
  STHIP_TEXEL_RGB8_UNORM = 18,
  STHIP_TEXEL_RGBA8_UNORM_ = 19, /* the same texels as 1 */
  STHIP_TEXEL_R8_SRGB = 20,
  STHIP_TEXEL_RG8_SRGB = 21,
  STHIP_TEXEL_RGB8_SRGB = 22,
  STHIP_TEXEL_RGBA8_SRGB = 23,
  STHIP_TEXEL_R16_UNORM = 24,
  STHIP_TEXEL_RG16_UNORM = 25,
  STHIP_TEXEL_RGB16_UNORM = 26,
  STHIP_TEXEL_RGBA16_UNORM = 27,
  STHIP_TEXEL_R32F = 28,
  STHIP_TEXEL_RG32F = 29,
  STHIP_TEXEL_RGB32F = 30,
  STHIP_TEXEL_RGBA32F_ = 31, /* the same texels as 0 */
  STHIP_TEXEL_BC1_RGB = 32,
  STHIP_TEXEL_BC2 = 33,
  STHIP_TEXEL_BC3 = 34,
  STHIP_TEXEL_BC4_UNORM = 35,
  STHIP_TEXEL_BC5_UNORM = 36,
  STHIP_TEXEL_BC1_RGB_SRGB = 37,
  STHIP_TEXEL_BC2_SRGB = 38,
  STHIP_TEXEL_BC3_SRGB = 39,
  STHIP_TEXEL_END = 40, /* one past the last format that is built */
  /* named and refused (STHIP_ERR_UNSUPPORTED) */
  STHIP_TEXEL_UNSUPPORTED_FIRST = 48,
  STHIP_TEXEL_BC4_SNORM = 48,
  STHIP_TEXEL_BC5_SNORM = 49,
  STHIP_TEXEL_BC6H_UFLOAT = 50,
  STHIP_TEXEL_BC6H_SFLOAT = 51,
  STHIP_TEXEL_BC7_UNORM = 52,
  STHIP_TEXEL_BC7_SRGB = 53,
  STHIP_TEXEL_R8_SNORM = 56, /* .. 59: R, RG, RGB, RGBA */
  STHIP_TEXEL_R16_SNORM = 60, /* .. 63 */
  STHIP_TEXEL_R8_UINT = 64, /* .. 67; 68 .. 71 SINT; 72 .. 75 16-bit UINT; 76 .. 79 16-bit SINT and wider integers, 64-bit */
  STHIP_TEXEL_UNSUPPORTED_END = 80
};
typedef struct sthip_decode_texels_desc {
  uint32_t src_format; /* sthip_texel_format */
  uint32_t width, height;
  uint32_t device_ptrs;
  uint32_t dst_format;   /* sthip_image_format: 0 binary32, 1 unorm8 */
  uint32_t dst_channels; /* 4: RGBA, 1: one channel */
  uint32_t channel;      /* 0 .. 3, which channel a one-channel destination takes; ignored with dst_channels 4 */
  uint32_t pad_;
  const void* src;
  void* dst;
} sthip_decode_texels_desc;
int sthip_decode_texels(sthip_ctx* ctx, const sthip_decode_texels_desc* desc);

/* ---- density grids from dense voxel arrays (load_volumes.cpp:87-91: GridBuilder<float>(0, FogVolume) over a dense box) ----
 * gVolumes[] takes finished NanoVDB 32.3 buffers. sthip_build_volume makes one ON THE DEVICE (volume_build.hip) from a dense
 * box of binary32 values, so that a host whose simulation leaves a dense array in device memory needs neither NanoVDB nor the
 * CPU. It stands alone, like sthip_convert_material: no scene is needed or touched, and the output is valid as
 * sthip_volume_desc::data of an upload. stratum_amd/nvdb.py (dense_to_nanovdb) states the same contract in numpy; the two
 * agree byte for byte.
 *
 * INPUT. dense[(x * dims[1] + y) * dims[2] + z], z fastest (a contiguous [nx, ny, nz] array, and NanoVDB's leaf order); dims
 * each >= 1; origin = the integer index coordinate of dense[0], may be negative and need not be a multiple of 8; voxel_size
 * and translation in binary64; an optional NUL-terminated name of at most 255 bytes. `dense` is a host pointer or, with
 * dense_is_device, a device pointer (4-byte aligned; rows that are 16-byte aligned take the wide loads).
 *
 * OUTPUT. One NanoVDB 32.3.3 float grid, class FogVolume, background 0, laid out as NanoVDB lays it out: GridData (672 B),
 * TreeData (64 B), the root (64 B) with its tiles (32 B each), then all upper nodes (270 400 B each), all lower nodes
 * (33 856 B), all leaves (2 144 B), breadth first. Every byte of the grid is written.
 *
 * RULES, each chosen so that every answer the readers use is GridBuilder's.
 *   - A voxel is active iff its value != 0 (GridBuilder::operator() skips v == background, so -0.0f is inactive and reads
 *     back as +0). Inactive voxels of an existing leaf hold 0; inactive tiles hold 0.
 *   - A leaf exists iff it has an active voxel; the same holds for a lower node, an upper node and a root tile. Root tiles are
 *     ordered ascending by signed tile coordinate (x, then y, then z: NanoVDB's std::map<Coord>). The nodes of a level follow
 *     their parents' order and then the child index.
 *   - Minimum, maximum and the index bounding box of the active voxels are exact at every level: leaf bbox_min / bbox_dif,
 *     node boxes, root box. The root maximum is the majorant of delta tracking, so it is the true maximum.
 *   - Average and standard deviation are written as 0. The grid flags claim bounding boxes, min/max and breadth-first order
 *     only (0x26). The checksum is all ones ("none"), the version word 0x04000c03.
 *   - STATED DIFFERENCE: GridBuilder turns a fully active constant leaf or lower node into a tile; this builder does not
 *     prune. Every lookup returns the same value either way.
 *   - Map: matf[i][i] = (float)voxel_size, invmatf[i][i] = (float)(1.0 / voxel_size), vecf = (float)translation; the binary64
 *     copies hold the unrounded values; both tapers are 1. World box: the binary64 map (index * voxel_size + translation,
 *     unfused) of the index box [min, max + 1]. Voxel size is written three times.
 * Refused with STHIP_ERR_INVALID_ARGUMENT before anything the caller owns is written: a NULL desc / dense / info, a struct_size
 * that is not sizeof(sthip_dense_volume_desc), a zero extent, a NaN or infinite value, no active voxel at all, a zero, negative
 * or non-finite voxel size, a non-finite translation, a name of more than 255 bytes, a box whose coordinates leave int32, a
 * box that touches more than 2^24 bricks of 8^3 voxels (2 048^3 voxels fit; the build's scratch is 20 B per brick), a grid of more than 0xFFFFFFF0 bytes, more than 65 536 root tiles, a device `out`
 * that is not 32-byte aligned.
 * TWO-CALL IDIOM: `info` is filled whenever the description passes; a capacity below info->bytes (or a NULL `out`) writes
 * nothing and returns STHIP_ERR_INVALID_ARGUMENT, so a first call with capacity 0 gives the size. With out_is_device the
 * grid is built in place in `out`; otherwise in a staging area of the context's and copied to the host. The call returns
 * synchronised. A library without the feature lacks the symbol. */
typedef struct sthip_dense_volume_desc {
  uint32_t struct_size; /* sizeof(sthip_dense_volume_desc) */
  uint32_t dense_is_device;
  const float* dense;
  uint32_t dims[3];
  int32_t origin[3];
  double voxel_size;
  double translation[3];
  const char* name; /* may be NULL */
} sthip_dense_volume_desc;
typedef struct sthip_volume_info {
  uint64_t bytes;                     /* of the grid */
  int32_t bbox_min[3], bbox_max[3];   /* index box of the active voxels (inclusive) */
  double world_bbox[6];               /* min xyz, max xyz: what a host needs for gViewMediumInstances */
  float min, max;                     /* over the active voxels */
  uint64_t active_voxels;
  uint32_t leaf_count, lower_count, upper_count, root_tiles;
  float device_ms; /* stream time of the kernels of the call (HIP events) */
  float call_ms;   /* wall time of the call */
} sthip_volume_info;
int sthip_build_volume(sthip_ctx* ctx, const sthip_dense_volume_desc* desc, void* out, uint64_t capacity, int out_is_device, sthip_volume_info* info);

/* ---- the grids of a resident scene ----
 * sthip_scene_set_volume replaces resident grid `volume_index` of gVolumes[] without an upload. The source is EITHER a finished
 * NanoVDB buffer (`data`, `bytes`; host memory, or device memory with data_is_device; checked exactly as the upload checks
 * it: magic, grid type, size, root and tile table inside the buffer) OR a dense description (`dense`, built on the device
 * into a staging area by the rules of sthip_build_volume). Every check and the build's read-back come first; a refusal
 * (STHIP_ERR_INVALID_ARGUMENT: no scene — STHIP_ERR_NO_SCENE —, an index out of range, a wrong struct_size, both or neither
 * source, anything the upload or sthip_build_volume refuses, grids beyond 16 GiB together) leaves the resident scene as it
 * was. Then, with no frame in flight, the install: the grids' words are laid out again back to back (so first_word may
 * change and a larger grid fits), the parsed header replaces the old one on the device and on the host, the entry boxes of
 * the volume instances that name the grid and the top level are made again by the path sthip_scene_update_transforms uses
 * (with the resident matrices), and with them the scene bounds. Kept reservoir grids ("reuse_grids_persist") are dropped, as
 * at an upload. With "keep_scene" the kept copy of the grid follows at once when the source is host bytes; otherwise it is
 * marked stale and fetched from the device immediately before anything is built again from the kept scene, by the rule
 * the environment and the images follow. If the top level cannot be made after the words were installed (STHIP_ERR_HIP,
 * STHIP_ERR_UNSUPPORTED), no scene is resident any more and the kept copy is dropped. The top level is the HOST-built one
 * afterwards, also where sthip_scene_set_transforms had built the resident one on the device. device_ms covers the build's
 * kernels and the copies of the install (HIP events); the top-level rebuild on the host, its copies and the read-back of the
 * resident matrices are part of call_ms only. `info` (may be NULL) is filled as by sthip_build_volume; for a
 * finished buffer only bytes, the index box, max and the times are known (the other fields are 0).
 * sthip_scene_read_volume copies what is resident: `*bytes` receives the grid's size (may be NULL); a `dst` of less capacity,
 * or NULL, is not written and gives STHIP_ERR_INVALID_ARGUMENT (two-call idiom). A library without the feature lacks the symbols. */
typedef struct sthip_volume_source {
  uint32_t struct_size; /* sizeof(sthip_volume_source) */
  uint32_t data_is_device;
  const void* data; /* a finished grid, or NULL */
  uint64_t bytes;
  const sthip_dense_volume_desc* dense; /* a dense box, or NULL */
} sthip_volume_source;
int sthip_scene_set_volume(sthip_ctx* ctx, uint32_t volume_index, const sthip_volume_source* source, sthip_volume_info* info);
int sthip_scene_read_volume(sthip_ctx* ctx, uint32_t volume_index, void* dst, uint64_t capacity, uint64_t* bytes);

/* ---- the environment of a resident scene (environment.h:8-25,96-150; dist2.h:80-154) ----
 * An image environment is three things in HBM: the RGBA32F image of gImages with its mip chain (Environment::sample_texel
 * descends it under eSampleEnvironmentMapDirectly), the four dist2d tables in gDistributions — marginal_pdf[H], row_pdf[H*W],
 * marginal_cdf[H+1], row_cdf[H*(W+1)] — and the Environment record in gMaterialData: ImageValue3 {value[3], image index} and,
 * with an image, the four table offsets. sthip_scene_set_environment replaces the value and / or the texels of the resident
 * environment and makes the mip chain and the tables again ON THE DEVICE (environment.hip); nothing else of the scene is
 * copied, rebuilt or analysed again.
 *   pixels != NULL: level 0 of the record's image is replaced (width x height must be the resident extent), every further
 *     level is made again, and the four tables are made again at the offsets the record names.
 *   pixels == NULL and value == NULL: the tables are made from the texels that are resident ("build the tables of what is
 *     resident": a host that uploaded zero-filled tables calls this once).
 *   value != NULL: the three floats of the record are rewritten, in gMaterialData on the device, in the context's host copy
 *     of it and in the kept scene. Alone it touches neither texels nor tables.
 * The trees, emitter tables and the material analysis stay as they are. The call does not count as a scene change for
 * "reuse_first_hits" (no triangle, instance or alpha mask moves: kept first hits stay valid); kept reservoir grids
 * ("reuse_grids_persist") are dropped, as at an upload. It waits for the stream and completes the frames in flight first, as
 * the other scene calls do, and returns when its own work on the stream has finished.
 *
 * The arithmetic is part of the contract; the results are the bits the host statements give (layout_images of
 * scene_prepare.cpp; build_distributions of scene.py and of stratum_hip.hpp).
 *   mip chain, all binary32: level k+1 has the extent max(1, w/2) x max(1, h/2); each channel of a texel is
 *     ((a + b) + (c + e)) * 0.25f over the texels (x0, y0), (x1, y0), (x0, y1), (x1, y1) of level k with
 *     x0 = min(2x, w-1), x1 = min(2x+1, w-1), y0 = min(2y, h-1), y1 = min(2y+1, h-1).
 *   tables, for the W x H texels of level 0:
 *     lum = (r*0.2126f + g*0.7152f) + b*0.0722f, binary32, unfused;
 *     s[y] = sin(M_PI * (y + 0.5f) * (1/(float)H)): y + 0.5f and 1/(float)H are binary32, the products and the sine binary64.
 *       The host part of the call computes the H values with libm and sends them up (no device sine equals libm's bits);
 *     f(x,y) = (double)lum * s[y];
 *     row[0] = 0; row[x+1] = (float)((double)row[x] + f(x,y)) for x = 0 .. W-1 in this order; integral = row[W];
 *     integral > 0: row[x] = row[x] / integral for x < W (a binary32 division), row_pdf[x] = (float)(f(x,y) / (double)integral);
 *     otherwise (zero, negative or NaN): row_pdf[x] = 1.0f / (float)W, row[x] = (float)x / (float)W, row[W] = 1;
 *     marginal: m[0] = 0; m[y+1] = m[y] + row_y[W] in y order, binary32 (a fallback row weighs 1); total = m[H];
 *     total > 0: marginal_cdf[y] = m[y] / total for y < H, marginal_pdf[y] = row_y[W] / total;
 *     otherwise: marginal_pdf[y] = 1.0f / (float)H, marginal_cdf[y] = (float)y / (float)H; in both cases marginal_cdf[H] = 1;
 *     last, row_y[W] = 1 for every row.
 *   Denormals are kept. Where a NaN stands is part of the contract; its sign and payload are not.
 * Only the x order of a row and the y order of the marginal are serial; the device runs one chain per lane for the rows
 * (k_env_rows), one lane for the marginal (k_env_marginal) and everything else elementwise (k_env_normalise, k_mip_rgba32f).
 *
 * Refusals are all decided before anything resident is touched; a refused call changes nothing.
 * STHIP_ERR_INVALID_ARGUMENT: no scene; a wrong struct_size; a material_address that is not a multiple of 4 or whose record
 * does not lie inside gMaterialData; an image index that is not in gImages; `pixels` for a record without an image; a width or
 * height that differs from the resident extent; a table that lies outside gDistributions (the check sthip_render makes) or
 * two tables of the record that overlap; a `value` of three zeros (upstream stores no record for a zero environment,
 * Scene.cpp:631-640). STHIP_ERR_UNSUPPORTED: the image is resident as RGBA8_UNORM (sthip_render refuses such an environment
 * too); `pixels` for an image that a material record of gMaterialData also names (the material analysis of the upload scanned
 * its texels: other texels could need other kernels).
 *
 * The kept scene ("keep_scene" = 1): a host `pixels` array and a `value` go into the kept copy at once. Pixels from a device
 * pointer and tables built on the device are NOT copied back per call: the kept image and the kept tables are marked stale and
 * fetched from the device immediately before anything is built again from the kept scene (a moved instance of the merged
 * mesh, a layout the refit does not serve, the failure fallback) — the rule the rigs follow. With "keep_scene" = 0 nothing is
 * kept and nothing needs doing.
 *
 * Cost, measured on an MI355X (profiles/r10/environment.json, tools/environment_times.py, medians of 9 calls, a small scene
 * under a 4096 x 2048 sky: 128 MB of texels, 64 MB of tables): 7.29 ms for the call with `pixels` in pageable host memory
 * (7.25 ms of it on the stream: the copy), 0.38 ms from a device pointer, 0.27 ms for the tables alone; the alternative
 * without this call is 38.9 ms for the host's build_distributions (one thread) plus 94.5 ms for sthip_scene_upload of the same
 * scene in the same process. Under a 2048 x 1024 sky: 1.86, 0.19 and 0.14 ms against 7.5 + 25.1 ms. The row pass is
 * latency-bound (0.18 ms, 0.18 of the triad rate, with 16 rows per wave, the default of "env_rows_per_wave"; 0.49 ms with 64).
 *
 * Measurement only: with the environment variable STHIP_ENVIRONMENT_TIMES=<file> (read once per process) every call that
 * builds tables appends one JSON line to the file with the HIP-event time of each stage: copy_ms, mips_ms, sines_ms,
 * k_env_rows_ms, k_env_marginal_ms, k_env_normalise_ms and the rows_per_wave in force (tools/environment_times.py reads them).
 * Without the variable the call makes no extra event and touches no file.
 *
 * sthip_scene_read_distributions: the resident gDistributions[first, first + count) copied to host memory after the work on
 * the stream has finished (tests; a host that wants device-built tables back). STHIP_ERR_INVALID_ARGUMENT: no scene, a range
 * past distribution_count, a NULL `out` with count > 0.
 * A library without the feature lacks the two symbols. */
typedef struct sthip_environment_desc {
  uint32_t struct_size;      /* sizeof(sthip_environment_desc) */
  uint32_t material_address; /* byte address of the Environment record in gMaterialData (what a render passes as gEnvironmentMaterialAddress) */
  const float* value;        /* 3 floats: new ImageValue3::value; NULL = keep */
  const void* pixels;        /* RGBA32F, width x height, tightly packed; NULL = keep the resident texels */
  uint32_t width, height;    /* with pixels: must equal the resident extent of the record's image */
  uint32_t device_ptr;       /* 1: pixels is device memory, readable in the order of the context's stream */
  uint32_t pad;
} sthip_environment_desc;
typedef struct sthip_environment_info { /* optional out-parameter, may be NULL */
  float device_ms;                      /* stream time of the copies and kernels of the call (HIP events) */
  float total_ms;                       /* wall time of the call */
} sthip_environment_info;
int sthip_scene_set_environment(sthip_ctx* ctx, const sthip_environment_desc* desc, sthip_environment_info* info);
int sthip_scene_read_distributions(sthip_ctx* ctx, uint32_t first, uint32_t count, float* out);

/* ---- the materials of a resident scene: texels and records ----
 * What a material looks like is two things in HBM: its record in gMaterialData (constants, and which images they bind) and the
 * texels of those images. sthip_scene_set_images replaces texels, sthip_scene_set_material_data replaces record bytes; neither
 * rebuilds a tree. Both follow the rules and the phase order of sthip_scene_set_environment: check (every refusal is decided on
 * the host before anything resident is touched, and a refused call changes nothing but sthip_last_error), reserve, wait for the
 * stream and complete the frames in flight, do the work on the stream, update the kept scene; they return when their work on
 * the stream has finished.
 *
 * Texels are not only data. The material analysis of the upload scans level 0 of the images that material records name for
 * their per-channel extremes, and decides from them whether some material of the scene can be specular. That decision caps
 * the bounce and shadow rounds of a render and lets k_shade end paths at gMaxDiffuseVertices, so texels replaced under a stale
 * analysis give wrong frames (a rough metal repainted as a mirror would lose every path beyond the diffuse budget). Both calls
 * therefore make the analysis again; for texels the scan is made again ON THE DEVICE (image_range.hip), wherever they came from.
 *
 * Image ranges (k_image_range), the contract — the bits of the upload's host scan but for the sign of a zero:
 *   lo[c] / hi[c] = the minimum / maximum of channel c over the texels of level 0 that are not NaN;
 *   an RGBA8_UNORM texel decodes as (float)b / 255.0f, which is monotone: the bytes are reduced and the result decoded once;
 *   bit c of nan_mask is set when some texel of channel c is a NaN; such a channel is unknown: lo[c] = -inf, hi[c] = +inf
 *     (a channel of nothing but NaNs included);
 *   infinities and denormals are kept as they are;
 *   the sign of a zero result is NOT part of the contract (-0 and +0 compare equal, and the analysis only compares ranges
 *     against 0.999f, 1e-2f and 0).
 * The device reduces with no floating-point atomics and no flags or spins inside a launch: one 16-byte load per lane per trip
 * of a grid-stride loop (one RGBA32F texel or four RGBA8 texels), running values in registers, cross-lane operations within a
 * wave, one LDS step per block, per-block partials with plain stores, and a second small launch that folds them; the kernel
 * boundary is the ordering. The results of all images of a call are read back once. The grid is sized from the device's CU count;
 * the option "image_range_blocks" forces the block count (tests) and never changes results.
 *
 * sthip_scene_set_images: `n` entries, applied together (the three images of one material change together). Each replaces
 * level 0 of gImages[index] (which = 0) or gImage1s[index] (which = 1) with `pixels`, width x height texels, tightly packed, in
 * the image's RESIDENT format (RGBA32F or RGBA8_UNORM; R32F or R8_UNORM) and at its resident extent: a change of extent or
 * format is an upload. device_ptr = 1: `pixels` is device memory, readable in the order of the context's stream (the outputs of
 * sthip_convert_material in its device form, for one). The mip chain of an image of gImages is made again on the device by the
 * rules of the upload (RGBA32F: ((a + b) + (c + e)) * 0.25f; RGBA8: (a + b + c + e + 2) >> 2); alpha masks have level 0 only.
 * Then every replaced image of gImages that a material record names is scanned, the analysis runs again on the host over the
 * resident records, and its has_specular is installed (nothing else of it can change through texels).
 *   Kept state: kept reservoir grids ("reuse_grids_persist") are dropped — stored samples carry the old materials' radiance.
 *   Kept first hits ("reuse_first_hits") stay when only images of gImages changed (no triangle or mask moved) and are dropped
 *   when an alpha mask changed (the alpha test decides first hits).
 *   An image that is also an environment's image: the library does not know that at this call. The dist2d tables stay as they
 *   were; the host follows with the tables-only form of sthip_scene_set_environment. (sthip_scene_set_environment itself still
 *   refuses texels for an image a material names.)
 *   The kept scene ("keep_scene" = 1): host pixels go into the kept copy at once; pixels from a device pointer mark the kept
 *   image stale, and it is fetched immediately before anything is built from the kept scene, as the environment's.
 *   Refused with STHIP_ERR_INVALID_ARGUMENT: no scene; a struct_size that is not sizeof(sthip_image_update); NULL `entries` with
 *   n > 0; a `which` above 1; an index out of range; NULL pixels; a width or height that differs from the resident extent; the
 *   same image named twice in one call; with device_ptr, a pointer that is not naturally aligned (16 bytes for RGBA32F, 4 for
 *   the other three formats).
 *
 * sthip_scene_set_material_data: the bytes [offset, offset + bytes) of gMaterialData are replaced by `data` (host memory);
 * offset and bytes are multiples of 4 and the range lies inside the resident buffer. For constants (base colour, emission
 * strength, metallic, roughness ...), for which image a value binds, and for medium parameters. The range goes into the
 * context's host copy, into the device buffer on the stream and into the kept scene; the analysis runs again and has_specular,
 * textured (which k_shade runs), the per-instance flags of k_cull_terminal and the set of images that materials name are
 * installed. An image that a record names for the first time is scanned on the device from its resident texels.
 * Kept reservoir grids are dropped; kept first hits stay.
 *   STHIP_ERR_INVALID_ARGUMENT: no scene, NULL data, a misaligned or outlying range; or, over the buffer as it would be after
 *   the edit, an instance's record that fails a material check of the upload (an image, bump map or alpha mask index that is
 *   out of range, a medium's volume index that is not in gVolumes).
 *   STHIP_ERR_UNSUPPORTED, because these entered the trees and tables at upload (upload the scene again): a triangle instance
 *   whose alpha_mask_index changes; a medium whose volume indices change; a triangle or sphere instance whose emission
 *   (base_color * emission > 0 in some channel) appears or disappears — the light list and the emitter bounds are the upload's.
 *
 * A range is the range of the texels that are resident: whatever replaces level 0 of an image of gImages (this call,
 * sthip_scene_set_environment) forgets the range the context held for it, also for an image that no record names at that moment;
 * the image is scanned again when a record names it.
 *   After the checks have passed, a failure of the device (STHIP_ERR_HIP: a copy, a launch, the read-back) can leave the texels
 *   or bytes of the call partly resident, with the material analysis and the ranges of the scene before the call and the kept
 *   reservoir grids dropped: the state is then not one any call describes, and the host uploads the scene again. The same holds
 *   for sthip_scene_set_material_data.
 *
 * sthip_scene_read_image_range: the range the context holds for gImages[image_index] (tests see the kernel's result through
 * it). STHIP_ERR_INVALID_ARGUMENT: no scene, an index out of range, or an image whose range nobody needed: one that no material
 * record names (any more), or names only under constants without a positive component (the upload does not scan those).
 *
 * Cost, measured on an MI355X (profiles/r11/material_update.json, tools/material_update_times.py, medians of 9 calls, a small
 * scene with one 4096 x 4096 parameter image): resident as RGBA8_UNORM (64 MB) 3.44 ms for sthip_scene_set_images with the
 * pixels in pageable host memory, 0.24 ms from a device pointer (0.26 ms for a sthip_convert_material and the call chained
 * behind it on the stream), against 0.14 + 36.4 + 41.9 ms for conversion, copy back and sthip_scene_upload_formats of the same
 * scene; resident as RGBA32F (256 MB) 13.5 ms and 0.55 ms against 0.28 + 139.6 + 218.0 ms. k_image_range alone, both launches:
 * 0.025 ms (RGBA8, 0.51 of the triad rate measured in the same process) and 0.068 ms (RGBA32F, 0.76 of it).
 *
 * Measurement only: with the environment variable STHIP_MATERIAL_TIMES=<file> (read once per process) every call that scans
 * appends one JSON line to the file with the HIP-event time of its k_image_range launches (k_image_range_ms), the images scanned
 * and the block count. Without the variable the call makes no extra event and touches no file.
 * A library without the feature lacks the three symbols. */
typedef struct sthip_image_update {
  uint32_t which;      /* 0 = gImages, 1 = gImage1s */
  uint32_t index;
  const void* pixels;  /* level 0 in the image's resident format, width x height, tightly packed */
  uint32_t width, height;
  uint32_t device_ptr; /* 1: pixels is device memory, readable in the order of the context's stream */
  uint32_t pad;
} sthip_image_update;
typedef struct sthip_images_info { /* optional out-parameter, may be NULL */
  float device_ms;                 /* stream time of the copies and kernels of the call (HIP events) */
  float total_ms;                  /* wall time of the call */
  uint32_t has_specular_before, has_specular_after; /* the analysis' verdict before and after the call (0 / 1) */
  uint32_t images_scanned;         /* images k_image_range ran over */
  uint32_t pad;
} sthip_images_info;
int sthip_scene_set_images(sthip_ctx* ctx, const sthip_image_update* entries, uint32_t n, uint32_t struct_size, sthip_images_info* info);
int sthip_scene_set_material_data(sthip_ctx* ctx, uint32_t offset, const void* data, uint32_t bytes, sthip_images_info* info);
int sthip_scene_read_image_range(sthip_ctx* ctx, uint32_t image_index, float lo[4], float hi[4], uint32_t* nan_mask);

/* ---- frame: replaces the dispatch sequence of BDPT::render (BDPT.cpp:607-720) ----
 * Renders seeds seed_begin .. seed_begin+seed_count-1 (gRandomSeed = seed, BDPT.cpp:480), one
 * sample per pixel centre per seed (bdpt.hlsl:167), and averages them with the running mean of
 * temporal_accumulation.hlsl:118-131. push_constants->gRandomSeed is ignored.
 *
 * sampling_flags are BDPTFlagBits (bdpt.h:12-44), scene_flags BDPT_FLAG_HAS_* (bdpt.h:46-49) as BDPT::render
 * resolves them (BDPT.cpp:486-541). Built: the default view-path integrator and, per flag, eAlphaTest, eNormalMaps,
 * eRayCones, eFlip*, eShadingNormalShadowFix, eUniformSphereSampling, eSampleEnvironmentMapDirectly, ePresampleLights,
 * eNEEReservoirs, eConnectToViews (sample_photons + add_light_trace), eConnectToLightPaths, and BDPT_FLAG_HAS_MEDIA
 * (volume instances over gVolumes). The flags whose upstream result depends on the order threads run in are built
 * with ONE defined order each: eLVC / eLVCReservoirs (cache filled in light-path
 * index order), eNEEReservoirReuse / eLVCReservoirReuse (hash-grid appends in (path, vertex) order; the seeds of a call
 * are then traced one at a time, seed s reading the grid of seed s - 1; not on a pixel-tile shard), eCoherentRR and
 * eCoherentSampling (the wave = the 8x4 pixel group, its first lane = the lowest lane that executes the statement).
 * Rejected with STHIP_ERR_UNSUPPORTED, never ignored: eSampleLightPower (reads an uninitialised table upstream) and the
 * combinations DESIGN.md section 5 lists (media exclude eCoherentSampling; light
 * subpaths and reuse exclude environments). Media without eDeferShadowRays are traced with k_shade walking every NEE ray itself.
 * ePerformanceCounters does not change results here; eRemapThreads only through the path index
 * (map_pixel_coord, bdpt_util.hlsli:76-83) that ePresampleLights and the light subpaths key on. */
int sthip_render(sthip_ctx* ctx, const sthip_BDPTPushConstants* push_constants, uint32_t sampling_flags,
                 uint32_t scene_flags, const sthip_frame_desc* frame, uint32_t seed_begin, uint32_t seed_count,
                 const sthip_outputs* outputs);

/* ---- pipelined host outputs: frame i + 1 renders while frame i copies back ----
 * sthip_render with host pointers renders, copies and synchronises inside the call, one after the other. The calls below
 * split that: sthip_render_async enqueues the frame and returns a ticket; the library renders it on the context's stream
 * into one of "output_ring" device staging sets and copies the set to the caller's host memory on a copy stream of its
 * own, ordered by events only (no kernel of this library moves the bytes: the runtime's device-to-host copy does, on a
 * copy engine or with its own copy kernel on a second hardware queue, beside the next frame's kernels); the caller
 * collects the frame later with sthip_wait_outputs. sthip_render itself is unchanged.
 *
 * sthip_host_alloc / sthip_host_free: pinned (page-locked) host memory of the context's device — the only kind a
 * device-to-host copy overlaps with anything. sthip_host_free first completes the frames in flight (one may still copy
 * into the block); blocks not freed are freed by sthip_destroy.
 *
 * sthip_render_async takes sthip_render's arguments and computes sthip_render's results: after sthip_wait_outputs(ticket)
 * the five images and gRayCount hold, byte for byte, what sthip_render with the same arguments writes (both
 * radiance_layouts, on a shard, with "half_color_precision"), and sthip_get_stats describes that frame. *ticket counts up
 * from 1.
 *   Argument lifetimes: push_constants, frame and everything frame points at are borrowed for the call only (the library
 *   keeps its own copy of the view arrays in pinned memory of the staging set). The host pointers inside `outputs` are
 *   borrowed until sthip_wait_outputs has returned for the ticket, or until the context is destroyed. gRayCount is
 *   written by the host when the ticket completes (sthip_wait_outputs, a sthip_outputs_ready that returns 1, or one of
 *   the draining calls below), from the frame's pinned counter record. outputs->device_ptrs must be 0 (the
 *   device-pointer form of sthip_render only enqueues already): otherwise STHIP_ERR_INVALID_ARGUMENT.
 *   Any host memory is correct; pinned memory overlaps: pointers from sthip_host_alloc, or memory the caller registered
 *   itself with hipHostRegister, get a true asynchronous copy. Pageable pointers still hold the right bytes at
 *   sthip_wait_outputs, but the runtime stages such a copy and the submit call may block until the frame is rendered.
 *   Ordering: tickets complete in submission order; sthip_wait_outputs(t) implies every earlier ticket is complete, and
 *   sthip_outputs_ready is monotone in the same way. A ticket that was never issued is STHIP_ERR_INVALID_ARGUMENT;
 *   waiting twice on the same ticket is STHIP_OK. The render work of all frames stays in one stream order, so the
 *   reservoir-reuse flags with "reuse_grids_persist" keep "N calls of one seed = one call of N seeds".
 *   What the submit call may wait for: in the steady state nothing on the GPU. Two exceptions: when "output_ring" frames
 *   are already in flight it waits for the COPY of the oldest one (its ticket stays valid and waitable); and on the
 *   out-of-memory retry (see sthip_render: the batch is halved) every frame in flight is completed before the path
 *   state is released.
 *   Rejected, never ignored, with STHIP_ERR_UNSUPPORTED and a sthip_last_error that says to use sthip_render:
 *   outputs->debug_mode != 0 (gDebugImage is in / out and chains from frame to frame through the caller's memory: a
 *   diagnostic mode, not a throughput mode) and "time_kernels" = 1 (its events synchronise the host).
 *   Other calls while frames are in flight: sthip_destroy, a sthip_set_stream that changes the stream, sthip_scene_upload,
 *   sthip_scene_update_transforms, sthip_host_free and a change of "output_ring" first complete every frame in flight
 *   (render and copy). After any of them except sthip_destroy the tickets stay waitable and waiting returns at once;
 *   after sthip_destroy the caller's buffers are complete and the tickets are gone with the context. A sthip_render or
 *   any other call between two async frames is legal and ordered after them on the stream. "half_color_precision" takes
 *   effect at the next submit; frames in flight keep the type they were submitted with.
 * sthip_outputs_ready: 1 = the frame's outputs are in host memory, 0 = not yet, < 0 = a sthip_status; never blocks.
 * sthip_wait_outputs: blocks until they are.
 * Option "output_ring" (1..8, default 2; other values are refused): frames in flight = device staging sets (the five
 * images: 64 B per pixel, 48 B with half colour precision — 132.7 MB at 1080p), allocated at first use, released when the
 * ring size or the frame size changes. A library without the feature answers STHIP_ERR_INVALID_ARGUMENT (unknown option):
 * a host may probe with it. */
int sthip_host_alloc(sthip_ctx* ctx, uint64_t bytes, void** out);
int sthip_host_free(sthip_ctx* ctx, void* p);
int sthip_render_async(sthip_ctx* ctx, const sthip_BDPTPushConstants* push_constants, uint32_t sampling_flags,
                       uint32_t scene_flags, const sthip_frame_desc* frame, uint32_t seed_begin, uint32_t seed_count,
                       const sthip_outputs* outputs, uint64_t* ticket);
int sthip_outputs_ready(sthip_ctx* ctx, uint64_t ticket);
int sthip_wait_outputs(sthip_ctx* ctx, uint64_t ticket);

/* Pixel-tile sharding for multi-GPU (one context per GPU): the frame is cut into
 * tile_w x tile_h tiles (multiples of the reference's 8x4 workgroup, bdpt.hlsl:11-12),
 * tile t is rendered iff t % shard_count == shard_rank; other pixels are written as zero
 * (including alpha) so that a sum-reduce over ranks assembles the frame.
 * shard_count = 1 (default) renders everything. */
int sthip_set_shard(sthip_ctx* ctx, uint32_t shard_rank, uint32_t shard_count, uint32_t tile_w, uint32_t tile_h);

/* The exchange step of a sharded frame without the zero padding: each rank renders with
 * outputs.radiance_layout = STHIP_LAYOUT_SHARD_TILES (sthip_shard_slot_count() float4 entries — 8-byte half4 entries
 * and a RGBA16F frame with "half_color_precision", bit-identical to the unsharded half frame — 1/shard_count of the
 * frame), the ranks' buffers are gathered on one GPU (RCCL gather / all_gather, rank r at packed + r * rank_stride
 * float4 entries; rank_stride >= rank 0's slot count, which is the largest), and sthip_assemble_tiles scatters them into
 * the W x H image on that GPU's context (device pointers, enqueued on the context's stream). */
uint32_t sthip_shard_slot_count(uint32_t width, uint32_t height, uint32_t shard_rank, uint32_t shard_count, uint32_t tile_w,
                                uint32_t tile_h);
int sthip_assemble_tiles(sthip_ctx* ctx, const float* packed, uint64_t rank_stride, uint32_t shard_count, uint32_t tile_w,
                         uint32_t tile_h, uint32_t width, uint32_t height, float* frame);
/* The same for the other outputs of a sharded frame (the G-buffer: albedo 16 B (8 B with half colour precision), VisibilityInfo 8 B, DepthInfo 16 B, prev-uv
 * 8 B per pixel), which sthip_render writes as W x H images that are zero outside the shard's tiles:
 * sthip_pack_tiles gathers the context's own tiles (its sthip_set_shard) out of such an image into slot order —
 * sthip_shard_slot_count() entries of entry_bytes each, the padding slots of edge tiles zero — and
 * sthip_assemble_tiles_bytes scatters the gathered buffers of all ranks (rank r at packed + r * rank_stride entries) into the
 * image. entry_bytes: a multiple of 4, at most 64. Device pointers; enqueued on the context's stream. */
int sthip_pack_tiles(sthip_ctx* ctx, const void* image, uint32_t width, uint32_t height, uint32_t entry_bytes, void* packed);
int sthip_assemble_tiles_bytes(sthip_ctx* ctx, const void* packed, uint64_t rank_stride, uint32_t shard_count, uint32_t tile_w,
                               uint32_t tile_h, uint32_t width, uint32_t height, uint32_t entry_bytes, void* frame);

/* The other way to spread a render call over GPUs: every GPU renders the WHOLE frame for its own part of the
 * seed range (sthip_set_shard(ctx, 0, 1, ..)), and the images are added up — one ncclReduce(sum) of the accumulation buffer.
 * It serves the estimators that build whole-frame structures (light tracing's splats, the reservoir-reuse hash grids), which
 * a tile shard cannot; the mean of N seeds then depends on the order of a floating-point sum (~1e-7 relative against the
 * one-GPU frame, where a tile shard is bit-identical). A call's radiance output is (mean over its seeds, their number):
 * sthip_radiance_to_sums turns `entries` RGBA32F entries in place into (sum over the seeds, their number), which a
 * sum-reduce can add; with back != 0 it turns such sums back into (mean, number). Device pointer; enqueued on the stream.
 * Returns STHIP_ERR_UNSUPPORTED while "half_color_precision" is on: a sum of rounded means is not a rounded mean. */
int sthip_radiance_to_sums(sthip_ctx* ctx, float* image, uint64_t entries, uint32_t back);

/* ---- the traversal contract on its own (T1/T2 of SURVEY.md §8a; intersection.hlsli:65-239) ---- */
typedef struct sthip_ray {
  float origin[3];
  float tmin;
  float direction[3];
  float tmax;
} sthip_ray;

typedef struct sthip_hit {
  float t; /* tmax of the ray on a miss */
  float b1, b2; /* barycentrics: P = v0 + b1 (v1-v0) + b2 (v2-v0), shading_data.hlsli:69-72 */
  uint32_t instance_primitive_index; /* 0xFFFFFFFF on a miss */
} sthip_hit;

/* any_hit bit 0 = 0: closest hit (trace_ray); 1: occlusion (RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH):
 * hits[i].instance_primitive_index is 0 when occluded, 0xFFFFFFFF when not; t,b1,b2 unspecified.
 * bit 1: alpha test on (gAlphaTest), bit 2: gFlipTriangleUVs for the mask lookup.
 * rays/hits are host pointers unless device_ptrs != 0. */
int sthip_trace_rays(sthip_ctx* ctx, const sthip_ray* rays, uint32_t ray_count, sthip_hit* hits, uint32_t any_hit,
                     uint32_t device_ptrs);

/* ---- the reuse hash grid on its own (test entry for the grid's defined order; hashgrid.hlsli:43-88) ----
 * The grids of eNEEReservoirReuse / eLVCReservoirReuse are built on the device. Their contents are DEFINED by a serial run:
 * the appends take effect in append order, append k probing the slots home .. home + 31 of a table of bucket_count + 32
 * slots (probing does not wrap) as the earlier appends left it — the first empty slot is claimed, the first slot that
 * holds the append's checksum is joined, an append that finds neither is dropped. counters[slot] is the number of appends
 * of the slot, indices its exclusive prefix sum in slot order, and dest[k] = indices[slot] + the rank of k among the slot's
 * appends in append order (0xFFFFFFFF for a dropped append). sthip_build_hash_grid runs the build a render runs — the same
 * kernels in the same order on the context's own buffers, with "hashgrid_serial" applying as it does in a render — and
 * copies the result to host memory. It needs a context and no scene. All pointers are host pointers. Two forms:
 *   form 0 (keys): keys[count] are (home bucket, checksum) pairs. The device arrays are sized by `slots` (>= count); the
 *     build bounds itself by the count in device memory, as in a render. `records`, `compacted_keys` and `data` are ignored.
 *   form 1 (NEE append records, 4 float4 each; staged when the last word of float4 2 — the cell size — is not zero as bits)
 *   form 2 (LVC append records, 6 float4 each; staged when the last word of float4 0 — the cell size — is not zero as bits):
 *     `records` holds `slots` records with holes. They are compacted in order, hashed (position = the first three words of
 *     float4 0, hashgrid_bucket_index), built, and scattered to `data` (3 resp. 5 float4 per record: NEE float4 0 =
 *     (r0.w, r1.x, r1.y, r1.z), 1 = (r2.x, r2.y, r2.z, r3.w), 2 = (r3.x, r3.y, r3.z, r1.w); LVC = float4 1..5 of the
 *     record). `keys` and `count` are ignored; info->count is the compacted count.
 * Outputs: checksums / counters / indices, bucket_count + 32 words each (checksum 0 = an empty slot); dest, of which the
 * first info->count words are written (the caller provides `count` words in form 0, `slots` otherwise); records forms only:
 * compacted_keys, 2 * slots words of which the first 2 * info->count are written, and data, slots * 3 (5) float4 — every
 * record the build did not place is zero. info: count; special_cells = the (home, checksum) cells that share their checksum
 * with a cell whose home is fewer than 32 slots away, as the device counted them; serial_rebuild
 * = 1 when the one-thread probe sequence built the table ("hashgrid_serial", or more than 1024 special cells); dropped =
 * the appends without a slot.
 * Refused with STHIP_ERR_INVALID_ARGUMENT before anything is touched (no device work, no output written): a NULL ctx, desc
 * or info; a struct_size that is not sizeof(sthip_hash_grid_desc); a form above 2; bucket_count outside (0, 2^28]; slots 0
 * or above 2^31 - 1; count > slots; a NULL pointer among those the form uses (keys may be NULL when count is 0); in form 0 a
 * home >= bucket_count or a checksum of 0 (0 marks an empty slot; hashgrid_bucket_index never produces it).
 * The call builds in the buffers a render keeps its grids in, so it DROPS the grids kept for the next render
 * ("reuse_grids_persist": the next render starts without a previous grid, as after a scene upload); it never hands a render a grid
 * of its own. It synchronises the context's stream. */
typedef struct sthip_hash_grid_desc {
  uint32_t struct_size; /* sizeof(sthip_hash_grid_desc) */
  uint32_t form;        /* 0 keys, 1 NEE append records, 2 LVC append records */
  uint32_t slots;
  uint32_t count;       /* form 0 */
  uint32_t bucket_count;
  uint32_t reserved0;
  const uint32_t* keys;  /* form 0: count x (home bucket, checksum) */
  const float* records;  /* forms 1, 2: slots x 4 (6) float4 */
  uint32_t* checksums;
  uint32_t* counters;
  uint32_t* indices;
  uint32_t* dest;
  uint32_t* compacted_keys; /* forms 1, 2 */
  float* data;              /* forms 1, 2 */
} sthip_hash_grid_desc;
typedef struct sthip_hash_grid_info {
  uint32_t count;
  uint32_t special_cells;
  uint32_t serial_rebuild;
  uint32_t dropped;
} sthip_hash_grid_info;
int sthip_build_hash_grid(sthip_ctx* ctx, const sthip_hash_grid_desc* desc, sthip_hash_grid_info* info);

/* ---- measurement ---- */
typedef struct sthip_stats {
  uint64_t rays_total;     /* gRayCount[0] semantics, last render */
  uint64_t rays_path;      /* gRayCount[1] semantics */
  uint64_t rays_shadow;
  uint64_t nodes_visited;  /* closest-hit rays; only when collected (sthip_set_option "count_traversal") */
  uint64_t tris_tested;
  uint64_t nodes_visited_shadow; /* any-hit (shadow) rays */
  uint64_t tris_tested_shadow;
  float ms_trace;          /* hipEvent time spent in the traversal kernel (k_trace) during the last render ("time_kernels") */
  float ms_shade;
  float ms_total;          /* all kernels of the last render */
  uint32_t launches_trace; /* k_trace launches of the last render */
  uint32_t bvh_node_bytes; /* bytes of one BVH node as laid out in HBM */
  uint32_t bvh_tri_bytes;  /* bytes of one leaf triangle */
  uint64_t bvh_nodes;
  uint64_t bvh_tris;
  float bvh_build_ms;      /* wall time of the acceleration-structure build inside the last sthip_scene_upload */
  float bvh_build_gpu_ms;  /* of which device time of the GPU builder's kernels ("bvh_builder" = 1) */
  /* lane-occupancy diagnostics of the trace kernels, [0] closest-hit, [1] shadow rays (with "count_traversal"):
   * 64 per wave-level iteration of the node loop / the triangle loop / per scheduling round of a persistent wave, and
   * the number of lanes that held a ray summed over rounds: nodes_visited / inner_slots etc. are lane utilisations */
  uint64_t inner_slots[2];
  uint64_t tri_slots[2];
  uint64_t round_slots[2];
  uint64_t busy_rounds[2];
  /* the first bounce runs as wave packets in a kernel of its own (k_trace_primary, "packet_primary" = 1): its share of
   * rays_path / nodes_visited / tris_tested, its launches and its time, all of which are NOT part of ms_trace /
   * launches_trace (so those describe k_trace alone). rays_primary_packets is what the packet kernel TRACED in the last
   * render: with "reuse_first_hits" it runs over one seed's paths when the kept hits do not fit the call, and not at all
   * when they do — 0 for a call served entirely from kept hits. Such rays are trace_ray calls of the reference all the
   * same: rays_total / rays_path / gRayCount count them as before */
  uint64_t rays_primary_packets;
  uint64_t nodes_visited_primary;
  uint64_t tris_tested_primary;
  float ms_trace_primary;
  uint32_t launches_primary;
  /* where the lanes of the persistent trace kernel are (with "count_traversal"; the 4-wide walk): summed over the wave-level
   * iterations of the node loop, the lanes [0] taking a node step, [1] waiting with a triangle leaf, [2] waiting with a
   * sentinel or an instance entry, [3] without a ray; [4] 64 per leaf phase, the lanes that [5] test a triangle and
   * [6] handle a sentinel or an entry in it; [7] 64 per refill stop of a wave */
  uint64_t lane_states[8];
  /* of rays_total / rays_path: last rays of paths — the path or diffuse budget ends at their far end, so they could only
   * still find an emitter — that missed the bounds of every emissive instance and were answered without a traversal
   * ("answer_last_rays" = 1, the default; scenes without images, spheres, environment or media). They are trace_ray calls of
   * the reference and are counted as such; nodes_visited etc. hold no visits for them */
  uint64_t rays_answered;
  /* the batch of the last render: paths of one seed on this shard, seeds traced together, the cap in force ("max_paths_in_flight":
   * sized at sthip_create from the device's FREE memory) and how often sthip_render has halved it because the device could not
   * hold a batch's state (a render retries with half the batch instead of failing with out-of-memory) */
  uint32_t paths_per_seed;
  uint32_t seeds_in_flight;
  uint64_t max_paths_in_flight;
  uint32_t batch_halvings;
  uint32_t full_rebuilds; /* sthip_scene_update_transforms calls that had to build the scene again (an instance of the merged mesh moved) */
  uint32_t leaf_records;  /* 1: the persistent trace kernel of the last render tested leaves from their 64-byte records ("leaf_pairs") */
  uint32_t reserved0;
} sthip_stats;
int sthip_get_stats(sthip_ctx* ctx, sthip_stats* out);

/* Measured memory-system ceilings for the roofline of the traversal kernel (bench.py): the rate, in GB/s, of
 *   STHIP_CEILING_TRIAD             a float4 stream triad over 3 x 512 MiB (the measured HBM figure SURVEY.md 8d asks for)
 *   STHIP_CEILING_NODE_GATHER_TABLE the traversal's own node fetch (64-byte BVH node per lane, 4 vector loads) at
 *                                   uniformly random nodes of the resident acceleration structure, with no dependence
 *                                   between fetches and no arithmetic: what L2 + Infinity Cache deliver to such gathers
 *   STHIP_CEILING_NODE_GATHER_L2    the same over a 2 MiB prefix of the node array (L2-hit rate)
 *   STHIP_CEILING_NODE_GATHER_L1    the same over a 16 KiB prefix (the vector-memory front end: nothing beats it)
 * counting 64 bytes per node fetch, as the algorithmic figure does. Synchronous; the gather kinds need a scene. */
enum { STHIP_CEILING_TRIAD = 0, STHIP_CEILING_NODE_GATHER_TABLE = 1, STHIP_CEILING_NODE_GATHER_L2 = 2, STHIP_CEILING_NODE_GATHER_L1 = 3 };
int sthip_measure_ceiling(sthip_ctx* ctx, uint32_t kind, double* gbytes_per_s);

/* named integer options: "count_traversal" (0/1), "time_kernels" (0/1); scheduler tuning of the persistent
 * trace kernels: "refill_idle" (1..64, default 16), "inner_min_lanes" (1..64, default 24),
 * "max_paths_in_flight" (how many seeds of the owned pixels are traced together; ~330 B of device memory per path at the default
 * flags; default: the largest power of two that leaves 4 KB of device memory per path, 2^26 on a 288 GB MI355X);
 * "bvh_builder": 0 = binned SAH on the host (default), 1 = the device-resident GPU builder (set before
 * sthip_scene_upload; a failed upload with it leaves the context without a scene), with "lbvh_algorithm" 1 = PLOC
 * (default) or 0 = Karras radix tree, "ploc_radius" (1..32, default 4) and "sah_top" (default 64: subtrees of at most that
 * many triangles keep their PLOC shape under a host-built SAH top; 0 = plain PLOC);
 * "wide_bvh" (the persistent trace kernel walks the tree collapsed into 4-wide nodes of 64 bytes with 8-bit child planes:
 * 1 = always (default) — host-built trees are collapsed on the host, the GPU builder's trees and the tree of a
 * transforms-only update on the device; 0 = never; 2 = only when the binary nodes exceed 4 MiB, one XCD's L2; 3 = the 8-wide
 * compressed form (80-byte nodes whose children are addressed by a base and a mask, 64-bit group stack) for host-built
 * trees, the 4-wide form for the others; not with "treetop" or "embed_leaves"), "tri_min_lanes" (1..64, default 1: the
 * 8-wide walk's leaf phase goes on while at least this many lanes hold a triangle), "leaf_pairs" (default 1: the persistent trace kernel tests a
 * leaf of a host-built 4-wide tree from one 64-byte record that holds the four vertices of its two edge-sharing triangles,
 * one memory round trip per leaf instead of one per triangle; 0 = from the per-triangle array, on the same tree. Takes effect
 * at the next render. The records take 64 bytes of device memory per leaf triangle, whatever the option says; a device that
 * cannot hold them renders without. Scenes with alpha masks or volumes and GPU-built trees have none and ignore the option;
 * a vertex update or a pose drops them until the next upload, a transforms-only update keeps them; sthip_stats::leaf_records
 * says whether the last render used them), "hashgrid_serial" (0/1: build the reservoir-reuse hash grids with the one-thread serial probe
 * sequence instead of the parallel device build: the same grids, for tests), "reuse_grids_persist" (default 0: every call starts a
 * new chain, its first seed finds no grid — upstream's first frame, gReservoirSpatialM = 0, BDPT.cpp:482-483. 1: the grids the
 * last seed of a call leaves are what the first seed of the NEXT call looks into, as long as that call asks for the same reuse
 * flags, gHashGridBucketCount, extent and gMaxDiffuseVertices — a host that renders one frame per call; N calls of one seed are
 * then one call of N seeds. Setting the option, to either value, also drops the kept grids (upstream: a frame whose camera moved
 * without reprojection), and so does sthip_scene_upload), "cull_terminal" (default 1: in a round where the
 * path or diffuse budget can end, only the paths that still have something to do reach the shading kernel), "answer_last_rays"
 * (default 1: a path's last ray is traced only if it can reach the bounds of an emissive instance; sthip_stats::rays_answered;
 * identical results for rays that start within a few scene sizes of the scene — as every path ray does — which is also what
 * the hit contract itself needs), "reuse_first_hits" (default 1: the primary ray of a pixel goes through its centre whatever the
 * seed, so the hits of the first bounce are kept on the device — 20 bytes per path of one seed, allocated at first use; a
 * device without room for them renders as with 0 — and traced again only when something they depend on changed: the views or
 * their transforms, the extent, the shard, whether gMaxPathVertices >= 2, eAlphaTest / eFlipTriangleUVs, or the scene, by any
 * of sthip_scene_upload, sthip_scene_update_transforms, sthip_scene_update_vertices, sthip_scene_animate, sthip_scene_set_rigs.
 * A host that renders one frame per call under a still camera traces the first bounce once; the seeds in flight of one call
 * share one trace. Frames, gRayCount and every stat but rays_primary_packets are the same either way. Setting the option, to
 * either value, drops the kept hits, and so do sthip_set_shard and a change of stream by sthip_set_stream. Not used under
 * "count_traversal" / "time_kernels", with volumes, or with "packet_primary" = 0),
 * "keep_scene" (default 1: a host copy of the uploaded arrays, see sthip_scene_update_transforms), "treetop" (default 0), "embed_leaves" (default 0), "lds_materials" (default 1), "lds_stack_levels" (4..150: LDS levels of the traversal stack; a higher
 * tree runs the bounded kernels, default: bounded at 32 levels beyond a height of 40): layout / scheduling options that
 * never change results, read at the next sthip_scene_upload / sthip_scene_update_transforms.
 *
 * An option that DOES change results: "half_color_precision" (0 = default, 1; other values are refused). While it is 1
 * the colour images of sthip_render (gRadiance, gAlbedo, gDebugImage; see sthip_outputs), sthip_tonemap (gInput,
 * gAlbedo, gOutput), sthip_accumulate (gRadiance, gAlbedo, gPrevAccumColor, gAccumColor), sthip_denoise_filter (gAccumColor, gFilterImages), sthip_image_compare (both
 * images) and sthip_assemble_tiles (8-byte entries) are RGBA16F; every other buffer keeps its type. It takes effect at
 * the next call. A library without the feature answers STHIP_ERR_INVALID_ARGUMENT (unknown option): a host may probe
 * with it.
 * "output_ring" (1..8, default 2): see sthip_render_async.
 * "denoise_block" (0 = default, 1): the lanes of a block of sthip_denoise_filter's kernels cover 32x8 or 16x16 pixels; never
 * changes results.
 * "env_rows_per_wave" (16 = default, or 64; anything else is refused): the rows a wave of k_env_rows owns in
 * sthip_scene_set_environment; never changes results.
 * "image_range_blocks" (0 = default: sized from the device's CU count; 1 .. 65535 force it; anything else is refused): the
 * blocks of k_image_range in sthip_scene_set_images / sthip_scene_set_material_data; never changes results. */
int sthip_set_option(sthip_ctx* ctx, const char* name, int64_t value);

/* ---- after the path: display transform, image metric, HDR export ---- */

/* Temporal accumulation of the renderer's output over frames, what Denoiser::denoise dispatches first
 * (src/Node/Denoiser.cpp:176-213 -> kernels/temporal_accumulation.hlsl:59-145): with `reprojection` the previous
 * frame's accumulated colour and luminance moments are fetched at gPrevUVs with a bilinear footprint whose taps must
 * pass the instance / normal / depth tests (:74-97), without it the same pixel is used (:102-109); then the new sample
 * is blended in with alpha = n_new / n, n clamped by history_limit (gHistoryLimit, 0 = unlimited). The binding names
 * are the shader's (denoiser.h). gViews is always a host pointer; the images are host pointers unless device_ptrs
 * (then, with up to 4 views, the call only enqueues its kernel on the context's stream: nothing is allocated or waited for).
 * (sthip_render's own N-seed mean is the same-pixel branch of this kernel applied seed by seed.)
 * With "half_color_precision" the four colour images are RGBA16F: read exactly, blended in binary32, gAccumColor rounded
 * to nearest even at its store; gAccumMoments stays RG32F and comes out as the binary32 call's on the upcast inputs. */
typedef struct sthip_accumulate_desc {
  uint32_t width, height;
  uint32_t view_count;        /* gViewCount */
  uint32_t reprojection;      /* specialisation constant gReprojection (Denoiser.cpp:76: on by default) */
  uint32_t demodulate_albedo; /* gDemodulateAlbedo: gRadiance.rgb /= 1e-2 + gAlbedo.rgb */
  float history_limit;        /* gHistoryLimit */
  uint32_t device_ptrs;
  uint32_t instance_count;    /* entries of gInstanceIndexMap */
  const sthip_ViewData* gViews;
  const float* gRadiance;                      /* RGBA32F (RGBA16F: half colour precision): rgb = sample, a = its sample count */
  const float* gAlbedo;                        /* RGBA32F (RGBA16F); may be NULL unless demodulate_albedo */
  const sthip_VisibilityInfo* gVisibility;     /* these five only with reprojection */
  const sthip_DepthInfo* gDepth;
  const float* gPrevUVs;                       /* RG32F */
  const sthip_VisibilityInfo* gPrevVisibility;
  const sthip_DepthInfo* gPrevDepth;
  const float* gPrevAccumColor;                /* RGBA32F (RGBA16F): rgb = mean so far, a = sample count */
  const float* gPrevAccumMoments;              /* RG32F: mean luminance, mean squared luminance */
  const uint32_t* gInstanceIndexMap;           /* SceneData::mInstanceIndexMap (Scene.cpp:383-385,414-418); NULL = identity */
  float* gAccumColor;                          /* out, RGBA32F (RGBA16F) */
  float* gAccumMoments;                        /* out, RG32F */
} sthip_accumulate_desc;
int sthip_accumulate(sthip_ctx* ctx, const sthip_accumulate_desc* desc);

/* FilterKernelType, src/Shaders/filter_type.h:8-16 */
enum {
  STHIP_FILTER_ATROUS = 0,
  STHIP_FILTER_BOX3,
  STHIP_FILTER_BOX5,
  STHIP_FILTER_SUBSAMPLED,
  STHIP_FILTER_BOX3_SUBSAMPLED,
  STHIP_FILTER_BOX5_SUBSAMPLED,
  STHIP_FILTER_TYPE_COUNT
};

/* The filter of the denoiser: what Denoiser::denoise dispatches after the temporal accumulation when mAtrousIterations > 0
 * (src/Node/Denoiser.cpp:215-265): estimate_variance (kernels/estimate_variance.hlsl:51-103) into gFilterImages[0], then
 * `iterations` passes of the edge-stopping filter (kernels/atrous.hlsl:211-262), pass i reading gFilterImages[i % 2] and
 * writing gFilterImages[(i + 1) % 2] with step 1 << i, and copy_rgb (:266-271) after pass history_tap - 1. The result
 * upstream returns is gFilterImages[iterations % 2]; after the call both images hold what upstream's ping-pong images hold.
 * Pixels outside every view are written by no pass (copy_rgb alone covers the whole extent).
 *
 * THE ARITHMETIC CONTRACT of the three passes. Everything is binary32, unfused, in the order written in the shaders
 * (include/sthip_detmath.h), with these decisions:
 *   max / saturate   max(a, K) with a constant K is `a > K ? a : K` (a NaN gives K); saturate(a) is `a > 0 ? (a < 1 ? a : 1) : 0`.
 *   length           length(v) of a float2 is sqrtf(v.x * v.x + v.y * v.y).
 *   powers           pow(d, 256) (atrous) and pow(d, 128) (variance) of the clamped normal dot product d are 8 and 7
 *                    successive squarings d = d * d. They are not det_powf: the base may be 0.
 *   exponential      a = -(w_l * w_l) - w_z (atrous) or a = -w_z (variance). A NaN `a` skips the tap. a < -87 makes w = 0:
 *                    the tap adds nothing (it is skipped: nothing is multiplied by that 0). Otherwise e = det_expf(a) and
 *                    w = e * kernel_weight * w_n, multiplied left to right (variance: w = e * w_n); then the shader's own
 *                    isinf(w) || isnan(w) skip.
 *   constants        kernel weights are the binary32 quotients of the literals: 2.0f/3.0f, 1.0f/6.0f, 4.0f/9.0f, 1.0f/9.0f,
 *                    1.0f/36.0f; the boxes and the subsampled kernel weigh every tap 1; compute_sigma_luminance's table
 *                    is {{1/4, 1/8}, {1/8, 1/16}}.
 *   helpers          luminance is dot(rgb, (0.2126, 0.7152, 0.0722)) added left to right; normals are bitfield.h's octahedral
 *                    unpack (det_f16tof32, the fold for z < 0, one division and three multiplies to normalise); a pixel's view
 *                    is the first whose [image_min, image_max) holds it, test_inside the same test — all as sthip_accumulate.
 *   tap order        sums are taken in the source order of atrous(), box3(), box5(), subsampled() (atrous.hlsl:121-207) and in
 *                    the yy-outer, xx-inner loops of estimate_variance and compute_sigma_luminance.
 *   accumulation     sum_color += color_p * (w, w, w, w * w); the result is sum_color * (1/sum_w, 1/sum_w, 1/sum_w,
 *                    (1/sum_w) * (1/sum_w)) with one division 1/sum_w.
 * Kept as upstream wrote it:
 *   - tap() receives an offset already multiplied by the step and multiplies it by the step again inside w_z's length(...)
 *     (atrous.hlsl:109). The product offset * step * step is taken as a SIGNED integer before the conversion to float (the
 *     unsigned reading of int * uint would make the filter asymmetric).
 *   - compute_sigma_luminance weighs the centre with kernel[1][1] = 1/16 (atrous.hlsl:87), and its 3x3 footprint does not
 *     scale with the step.
 *   - copy_rgb always reads gFilterImages[0], whichever image the tapped iteration wrote (atrous.hlsl:270).
 *   - estimate_variance maps the centre's instance index through gInstanceIndexMap but compares it with a neighbour of the
 *     CURRENT frame (estimate_variance.hlsl:83). An index beyond instance_count maps to 0xFFFFFFFF (matches nothing).
 *   - pixels whose z is infinite (misses: the renderer writes inf) go through sigma_l and the division by sum_w = 1 only.
 *   - a tap whose w is 0 through w_n = 0 is NOT skipped: 0 * (a NaN or inf colour) reaches the sum, as upstream.
 * Upstream defect, noted only: Denoiser.cpp:225 pushes the TEMPORAL pipeline's constants to the variance dispatch, so
 * gVarianceBoostLength never reaches the shader (and gHistoryLimit does only because the offsets coincide). Here
 * variance_boost_length is an explicit field, 0 = off.
 *
 * gViews is always a host pointer. Host form (device_ptrs = 0): the inputs are staged, both filter images are copied back,
 * gAccumColor too when the tap fired (1 <= history_tap <= iterations), and the call returns synchronised. Device form: the
 * passes are only enqueued on the context's stream, one after another (the kernel boundary is their only synchronisation);
 * with up to 4 views nothing is staged or waited for. The filter taps read a per-pixel guide image {n.x, n.y, n.z, z} (16 B:
 * the unpacked normal and the depth, exactly the values named above) that estimate_variance writes; it is scratch the context
 * owns and the one allocation the device form can make: it grows only when the extent exceeds every earlier call's.
 * With "half_color_precision" gAccumColor and both filter images are RGBA16F, as upstream's are (Denoiser.cpp:160-163): every
 * pass reads halves exactly, computes in binary32 and rounds to nearest even at its one store; gAccumMoments, gVisibility and
 * gDepth keep their types.
 * Refused with STHIP_ERR_INVALID_ARGUMENT, the message naming the field: a NULL gViews / gVisibility / gDepth / gAccumColor /
 * gAccumMoments / gFilterImages[k], view_count = 0, iterations outside 1..8, filter_type >= 6, an empty extent or one of more
 * than 2^31 - 1 pixels, a view of gViews whose [image_min, image_max) leaves the extent (the taps are bounded by their view). */
typedef struct sthip_denoise_desc {
  uint32_t width, height;
  uint32_t view_count;         /* gViewCount */
  uint32_t device_ptrs;
  uint32_t instance_count;     /* entries of gInstanceIndexMap */
  uint32_t iterations;         /* mAtrousIterations, 1..8; pass i has gIteration = i, gStepSize = 1 << i */
  uint32_t filter_type;        /* specialisation constant gFilterKernelType (STHIP_FILTER_*; upstream's default is BOX3) */
  uint32_t history_tap;        /* mHistoryTap: copy_rgb after pass history_tap - 1; 0 or > iterations: never */
  float history_limit;         /* gHistoryLimit of estimate_variance: pixels with at least this many samples take their own moments */
  float variance_boost_length; /* gVarianceBoostLength, 0 = off */
  float sigma_luminance_boost; /* gSigmaLuminanceBoost (upstream's default: 3, Denoiser.cpp:75) */
  uint32_t pad_;
  const sthip_ViewData* gViews;
  const sthip_VisibilityInfo* gVisibility;
  const sthip_DepthInfo* gDepth;
  const uint32_t* gInstanceIndexMap; /* NULL = identity */
  float* gAccumColor;                /* in; out as well when the tap fires. RGBA32F (RGBA16F) */
  const float* gAccumMoments;        /* in, RG32F */
  float* gFilterImages[2];           /* out, RGBA32F (RGBA16F): rgb = colour, a = variance */
  /* optional, host memory, 10 floats, for measurements: when not NULL every pass is bracketed by events and the call waits
   * for them: milliseconds of [0] estimate_variance, [1 + i] pass i, [9] copy_rgb (0 for passes that did not run) */
  float* pass_ms;
} sthip_denoise_desc;
int sthip_denoise_filter(sthip_ctx* ctx, const sthip_denoise_desc* desc);

/* TonemapMode, src/Shaders/tonemap.h:8-21 */
enum {
  STHIP_TONEMAP_RAW = 0,
  STHIP_TONEMAP_REINHARD,
  STHIP_TONEMAP_REINHARD_EXTENDED,
  STHIP_TONEMAP_REINHARD_LUMINANCE,
  STHIP_TONEMAP_REINHARD_LUMINANCE_EXTENDED,
  STHIP_TONEMAP_UNCHARTED2,
  STHIP_TONEMAP_FILMIC,
  STHIP_TONEMAP_ACES,
  STHIP_TONEMAP_ACES_APPROX,
  STHIP_TONEMAP_VIRIDIS_R,
  STHIP_TONEMAP_VIRIDIS_LENGTH_RGB,
  STHIP_TONEMAP_MODE_COUNT
};

/* What BDPT::render binds and pushes for its "tone map" block (src/Node/BDPT.cpp:783-815, kernels/tonemap.hlsl:7-19):
 * specialisation constants gMode / gModulateAlbedo / gGammaCorrection, push constant gExposure, images gInput,
 * gAlbedo, gOutput (RGBA32F, width*height). The two dispatches of the reference (clear gMax + reduce_max, then main)
 * happen inside one call. gExposureAlpha (smoothing of the maxima over frames, default 0 = off) is not taken: every
 * call uses the maxima of its own input. out_max (optional, host memory, 4 floats) receives the rgb and luminance
 * maxima main() sees. With "half_color_precision" gInput, gAlbedo and gOutput are RGBA16F: the inputs are read exactly,
 * gOutput is rounded to nearest even at its store; out_max and exposure_state are those of the binary32 call on the
 * upcast inputs. */
typedef struct sthip_tonemap_desc {
  uint32_t width, height;
  uint32_t mode;
  uint32_t modulate_albedo;
  uint32_t gamma_correction;
  float exposure;
  uint32_t device_ptrs; /* gInput/gAlbedo/gOutput are device pointers */
  float exposure_alpha; /* gExposureAlpha (tonemap.hlsl:169-178): in (0, 1) the maxima the curves use are blended with the
                           previous frame's, lerp(prev, cur, alpha) (the luminance moments with sqrt(alpha)); needs exposure_state */
  const float* gInput;
  const float* gAlbedo; /* may be NULL when modulate_albedo == 0 */
  float* gOutput;
  float* out_max;
  /* host, in/out, may be NULL: what the reference keeps at bytes 16..39 of gMax / reads from gPrevMax — the (blended)
   * maxima r, g, b, luminance and the two luminance moments of the previous call; all zero before the first frame */
  float* exposure_state;
} sthip_tonemap_desc;
int sthip_tonemap(sthip_ctx* ctx, const sthip_tonemap_desc* desc);

/* ImageCompareMode, kernels/image_compare.hlsl:5-9 */
enum { STHIP_COMPARE_SMAPE = 0, STHIP_COMPARE_MSE = 1, STHIP_COMPARE_AVERAGE = 2 };

/* The metric ImageComparer shows (src/Node/ImageComparer.cpp:61-90 dispatching kernels/image_compare.hlsl:13-46):
 * per-pixel error over rgb, divided by 3*width*height, summed per group of 64 consecutive pixels, scaled by
 * `quantization` (gQuantization; the node's default is 1024, ImageComparer.hpp:18), truncated to uint and added atomically.
 * sum_out = the raw uint accumulator, overflow_out = the overflow flag; the displayed number is sum/quantization
 * (its square root for MSE, ImageComparer.cpp:88). image1/image2: RGBA32F (RGBA16F with "half_color_precision", read
 * exactly: the sums of the binary32 call on the upcast images), host unless device_ptrs. */
int sthip_image_compare(sthip_ctx* ctx, const float* image1, const float* image2, uint32_t width, uint32_t height, uint32_t metric, uint32_t quantization,
                        uint32_t device_ptrs, uint32_t* sum_out, uint32_t* overflow_out);

/* Radiance .hdr export of an RGBA32F host image (always RGBA32F: a half image is upcast by the caller), what BDPT's "Export HDR" does through stbi_write_hdr(path, w, h, 4,
 * pixels) (src/Node/BDPT.cpp:313-337): header "#?RADIANCE", FORMAT=32-bit_rle_rgbe, rows top to bottom, RGBE with
 * the shared exponent of the largest channel; rows of 8..32767 pixels are run-length coded per channel, others flat.
 * Host-only, needs no context. Returns STHIP_OK or STHIP_ERR_INVALID_ARGUMENT (bad arguments / cannot write). */
int sthip_write_hdr(const char* path, uint32_t width, uint32_t height, const float* rgba);

#ifdef __cplusplus
}
#endif
#endif /* STHIP_H */
