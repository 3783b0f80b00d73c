// context.h — private to the units of the C ABI (api.hip, post.hip): the context struct with the types it is made of and the
// error macros. It includes no kernel: kernels.h and kernel_instances.h are api.hip's alone (traverse.h is here for DeviceBvh).
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <map>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/sthip.h"
#include "bvh_build.h"
#include "environment.h"
#include "first_hits.h"
#include "kernel_constants.h"
#include "scene_prepare.h"
#include "top_level.h"
#include "traverse.h"
#include "vertex_streams.h"
#include "volume_build.h"

// (nothing in here is part of the library's interface: the types and the functions stay out of its dynamic symbol table)
#pragma GCC visibility push(hidden)

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }  // an early return (HIP_TRY) must not leak a local staging buffer
  hipError_t ensure(size_t count) {
    if (count <= n && p) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    if (count == 0) return hipSuccess;
    hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
    if (e == hipSuccess) n = count;
    // tests: STHIP_POISON_ALLOC=<byte> fills every new device buffer with that byte, so that a read of something nothing has
    // written shows in a fresh process too (where new device memory is zero pages) and not only once the heap is recycled
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
// The unpacked nodes the host keeps (treetop selection, top-level rebuilds): page-locked, so that the device-resident
// builder's one node copy runs at PCIe speed, and never zero-filled
struct PinnedNodes {
  BvhNode* p = nullptr;
  size_t n = 0, cap = 0;
  PinnedNodes() = default;
  PinnedNodes(const PinnedNodes&) = delete;
  PinnedNodes& operator=(const PinnedNodes&) = delete;
  ~PinnedNodes() {
    if (p) (void)hipHostFree(p);
  }
  hipError_t ensure(size_t count) {  // capacity only; contents are lost when it grows
    if (count <= cap && p) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = n = 0;
    hipError_t e = hipHostMalloc((void**)&p, std::max<size_t>(1, count) * sizeof(BvhNode), hipHostMallocDefault);
    if (e == hipSuccess) cap = std::max<size_t>(1, count);
    return e;
  }
  bool empty() const { return n == 0; }
  size_t size() const { return n; }
  BvhNode* data() { return p; }
};

// The scene as it was uploaded, kept on the host ("keep_scene" = 1, the default): what a change that the resident tree cannot
// follow — an instance of the merged world-space mesh that moves — is rebuilt from, inside sthip_scene_update_transforms
// (the reference rebuilds whatever is dirty, Scene.cpp:345,435-459,614-629: it has the scene graph to rebuild from).
struct KeptScene {
  std::vector<sthip_PackedVertexData> vertices;
  std::vector<uint8_t> indices, materials;
  std::vector<sthip_InstanceData> instances;
  std::vector<sthip_TransformData> xf, inv, motion;
  std::vector<uint32_t> lights;
  std::vector<std::vector<float>> image_pixels, image1_pixels;
  std::vector<std::vector<uint8_t>> image_bytes, image1_bytes;  // the 8-bit images, as they came: bytes (the float vector of such an image stays empty)
  std::vector<uint8_t> image_formats, image1_formats;           // sthip_image_format per image (sthip_scene_upload_formats)
  std::vector<sthip_image_desc> images, images1;
  std::vector<float> distributions;
  std::vector<std::vector<uint8_t>> volume_bytes;
  std::vector<sthip_volume_desc> volumes;
  bool valid = false;
  // How far the copy lags behind the device; upload_kept_scene fetches all of it before anything is built from the copy.
  // ranges [first, end) of the vertices that an animate call left behind the device's (sync_kept_vertices)
  std::vector<std::pair<uint32_t, uint32_t>> stale_vertices;
  // the images (gImages / gImage1s, in either format) whose texels came from a device pointer and are newer on the device
  // (sthip_scene_set_environment, sthip_scene_set_images), and the tables sthip_scene_set_environment built on the device
  // (sync_kept_environment)
  std::set<uint32_t> stale_images, stale_images1;
  bool stale_env_tables = false;
  // the grids of gVolumes that sthip_scene_set_volume built on the device or took from a device pointer (sync_kept_volumes)
  std::set<uint32_t> stale_volumes;
  // The host wrote the kept records [first, first + count): they are not stale any more
  void vertices_written(uint32_t first, uint32_t count) {
    if (stale_vertices.empty() || !count) return;
    const uint32_t end = first + count;
    std::vector<std::pair<uint32_t, uint32_t>> left;
    for (const auto& r : stale_vertices) {
      if (end <= r.first || r.second <= first) {
        left.push_back(r);
        continue;
      }
      if (r.first < first) left.emplace_back(r.first, first);
      if (end < r.second) left.emplace_back(end, r.second);
    }
    stale_vertices.swap(left);
  }
  void keep(const sthip_scene_desc& s, const uint8_t* formats, const uint8_t* formats1) {
    vertices.assign(s.gVertices, s.gVertices + (s.gVertices ? s.vertex_count : 0));
    indices.assign((const uint8_t*)s.gIndices, (const uint8_t*)s.gIndices + (s.gIndices ? s.indices_bytes : 0));
    materials.assign((const uint8_t*)s.gMaterialData, (const uint8_t*)s.gMaterialData + (s.gMaterialData ? s.material_bytes : 0));
    instances.assign(s.gInstances, s.gInstances + s.instance_count);
    xf.assign(s.gInstanceTransforms, s.gInstanceTransforms + s.instance_count);
    inv.assign(s.gInstanceInverseTransforms, s.gInstanceInverseTransforms + s.instance_count);
    motion.clear();
    if (s.gInstanceMotionTransforms) motion.assign(s.gInstanceMotionTransforms, s.gInstanceMotionTransforms + s.instance_count);
    lights.assign(s.gLightInstances, s.gLightInstances + (s.gLightInstances ? s.light_count : 0));
    auto take = [](const sthip_image_desc* in, uint32_t n, size_t channels, const uint8_t* formats, std::vector<std::vector<float>>& px, std::vector<std::vector<uint8_t>>& bytes, std::vector<uint8_t>& fmt,
                   std::vector<sthip_image_desc>& d) {
      px.assign(n, {});
      bytes.assign(n, {});
      fmt.assign(n, 0);
      d.assign(n, sthip_image_desc{});
      for (uint32_t i = 0; i < n; i++) {
        const size_t count = (size_t)in[i].width * in[i].height * channels;
        fmt[i] = formats ? formats[i] : 0;
        if (fmt[i]) {  // 8-bit: `pixels` points at bytes
          const uint8_t* b = reinterpret_cast<const uint8_t*>(in[i].pixels);
          bytes[i].assign(b, b + count);
          d[i] = sthip_image_desc{reinterpret_cast<const float*>(bytes[i].data()), in[i].width, in[i].height};
        } else {
          px[i].assign(in[i].pixels, in[i].pixels + count);
          d[i] = sthip_image_desc{px[i].data(), in[i].width, in[i].height};
        }
      }
    };
    take(s.gImages, s.gImages ? s.image_count : 0, 4, formats, image_pixels, image_bytes, image_formats, images);
    take(s.gImage1s, s.gImage1s ? s.image1_count : 0, 1, formats1, image1_pixels, image1_bytes, image1_formats, images1);
    distributions.assign(s.gDistributions, s.gDistributions + (s.gDistributions ? s.distribution_count : 0));
    volume_bytes.assign(s.gVolumes ? s.volume_count : 0, {});
    volumes.assign(volume_bytes.size(), sthip_volume_desc{});
    for (size_t i = 0; i < volume_bytes.size(); i++) {
      volume_bytes[i].assign((const uint8_t*)s.gVolumes[i].data, (const uint8_t*)s.gVolumes[i].data + s.gVolumes[i].bytes);
      volumes[i] = sthip_volume_desc{volume_bytes[i].data(), s.gVolumes[i].bytes};
    }
    valid = true;
    stale_vertices.clear();  // (what is kept now is what is resident)
    stale_images.clear();
    stale_images1.clear();
    stale_env_tables = false;
    stale_volumes.clear();
  }
  void set_transforms(const sthip_TransformData* new_xf, const sthip_TransformData* new_inv, const sthip_TransformData* new_motion, uint32_t n) {  // (motion NULL: identity)
    xf.assign(new_xf, new_xf + n);
    inv.assign(new_inv, new_inv + n);
    motion.clear();
    if (new_motion) motion.assign(new_motion, new_motion + n);
  }
  sthip_scene_desc desc() const {
    sthip_scene_desc d{};
    d.gVertices = vertices.data();
    d.vertex_count = (uint32_t)vertices.size();
    d.gIndices = indices.data();
    d.indices_bytes = (uint32_t)indices.size();
    d.gInstances = instances.data();
    d.instance_count = (uint32_t)instances.size();
    d.gInstanceTransforms = xf.data();
    d.gInstanceInverseTransforms = inv.data();
    d.gInstanceMotionTransforms = motion.empty() ? nullptr : motion.data();
    d.gMaterialData = materials.data();
    d.material_bytes = (uint32_t)materials.size();
    d.gLightInstances = lights.data();
    d.light_count = (uint32_t)lights.size();
    d.gImages = images.empty() ? nullptr : images.data();
    d.image_count = (uint32_t)images.size();
    d.gDistributions = distributions.empty() ? nullptr : distributions.data();
    d.distribution_count = (uint32_t)distributions.size();
    d.gImage1s = images1.empty() ? nullptr : images1.data();
    d.image1_count = (uint32_t)images1.size();
    d.gVolumes = volumes.empty() ? nullptr : volumes.data();
    d.volume_count = (uint32_t)volumes.size();
    return d;
  }
};

// One frame in flight of sthip_render_async: a device staging set of the five images, the copy of the call's view arrays in
// pinned memory (the arguments are borrowed for the call only), the frame's counters on the device and in a pinned record,
// and the two events that order it: `rendered` on the render stream, `copied` on the copy stream.
struct AsyncSlot {
  DevBuf<float4> radiance, albedo;
  DevBuf<sthip_VisibilityInfo> visibility;
  DevBuf<sthip_DepthInfo> depth;
  DevBuf<float2> prev_uv;
  DevBuf<unsigned long long> counters;
  size_t key[3] = {0, 0, 0};  // (pixels, radiance entries, bytes per colour entry) the set was allocated for
  uint8_t* params = nullptr;  // pinned: gViews | gViewTransforms | gPrevViews | gPrevInverseViewTransforms | gInverseViewTransforms | gViewMediumInstances
  size_t params_cap = 0;
  unsigned long long* record = nullptr;  // pinned: CNT_TOTAL counters of the frame
  hipEvent_t rendered = nullptr, copied = nullptr;
  uint64_t ticket = 0;            // the ticket in flight in this slot, 0 = free
  uint64_t* ray_count = nullptr;  // the caller's gRayCount: written from `record` when the ticket is retired
  AsyncSlot() = default;
  AsyncSlot(const AsyncSlot&) = delete;
  AsyncSlot& operator=(const AsyncSlot&) = delete;
  ~AsyncSlot() {
    if (params) (void)hipHostFree(params);
    if (record) (void)hipHostFree(record);
    if (rendered) (void)hipEventDestroy(rendered);
    if (copied) (void)hipEventDestroy(copied);
  }
  void release_images() {
    radiance.release();
    albedo.release();
    visibility.release();
    depth.release();
    prev_uv.release();
    key[0] = key[1] = key[2] = 0;
  }
};

struct sthip_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string error;
  int cu_count = 256;
  // scene
  bool has_scene = false;
  bool textured = false;      // some material binds an image: k_shade<true> (ray cones, image values, normal maps)
  bool has_alpha = false;     // some triangle material has an alpha mask (gImage1s)
  bool has_spheres = false;   // some instance is a sphere: k_shade<., true>
  bool has_volumes = false;   // some instance is a volume (a Medium): the media instantiations
  uint32_t volume_count = 0, volume_instances = 0;
  std::vector<uint8_t> instance_is_volume;
  sthip::TopLevelState top;  // what sthip_scene_update_transforms rebuilds the top level from
  KeptScene kept;            // ... and what it rebuilds everything from when the top level alone cannot follow the change
  bool keep_scene = true;    // "keep_scene"
  size_t nodes_capacity = 0;
  DevBuf<uint32_t> volume_words;
  DevBuf<DeviceVolume> volumes;
  std::vector<uint8_t> materials_host;                    // gMaterialData as uploaded (validation of the environment record)
  std::vector<std::pair<uint32_t, uint32_t>> image_dims;  // (width, height) of gImages
  uint32_t distribution_count = 0;
  bool has_specular = false;  // some material satisfies DisneyMaterial::is_specular (disney_material.hlsli:125)
  DevBuf<sthip_PackedVertexData> vertices;
  DevBuf<uint8_t> indices;
  DevBuf<sthip_InstanceData> instances;
  DevBuf<sthip_TransformData> xf, inv_xf, motion_xf;
  DevBuf<uint8_t> materials;
  DevBuf<uint32_t> lights;
  DevBuf<DeviceImage> images;
  DevBuf<float4> image_texels;
  DevBuf<uint32_t> image_texels8;        // the RGBA8 images' texels (a word per texel), every level; DeviceImage::offset indexes it for them
  std::vector<DeviceImage> images_host;  // the table as uploaded (sthip_scene_read_image; the environment's format at render)
  uint32_t image_count = 0;
  DevBuf<float2> cone;
  uint32_t instance_count = 0, light_count = 0;
  DevBuf<BvhNodeSlot> nodes;
  DevBuf<BvhTri> tris;
  DevBuf<TlasEntry> entries;
  DevBuf<WideNode> wide_nodes;
  DevBuf<TlasEntry> wide_entries;
  // "leaf_pairs": the leaf records of a host-built 4-wide tree (bvh.h: LeafPair), made at upload. 1 (default): k_trace tests
  // leaves from them while they are resident; 0: from BvhTri, on the same tree. Anything that moves leaf triangles on the
  // device drops them (api.hip: drop_leaf_pairs).
  DevBuf<LeafPair> pairs;
  bool leaf_pairs = true, leaf_pairs_resident = false;
  DevBuf<Wide8Node> wide8_nodes;
  DevBuf<TlasEntry> wide8_entries;
  std::vector<Wide8Node> wide8_host;  // the 8-wide nodes as uploaded: a transforms-only update makes the top level's again behind the bottom levels'
  size_t wide8_node_count = 0;
  uint32_t tri_min_lanes = 1;  // "tri_min_lanes" (DeviceBvh::wide8_tri_min)
  DeviceBvh bvh{};
  uint64_t bvh_nodes = 0, bvh_tris = 0;
  // treetop (bvh_build.h): rebuilt whenever the top level changes; needs the nodes on the host
  PinnedNodes nodes_host;
  DevBuf<BvhNode> raw_nodes;  // device-resident build only: the unpacked nodes before their one copy to nodes_host
  DevBuf<BvhNodePacked> top_nodes;
  DevBuf<TlasEntry> top_entries;
  bool use_treetop = false;  // "treetop": measured +1.5 % before k_trace's loop lost its other exec-mask regions, -0.5 % after
  // host builds: leaf triangles in the node array behind their parent (bvh_build.h: BuiltBvh::embedded). Measured on the
  // bench scene: k_trace 2.30 ms either way (the leaf fetch is not what a step waits for), so off: two arrays are simpler
  bool embed_leaves = false;
  // "wide_bvh": k_trace walks the 4-wide form of the tree (takes effect at the next sthip_scene_upload). 1 (default) = always:
  // host-built trees are collapsed on the host, GPU-built ones and the trees of a transforms-only update on the device
  // (wide.hip). 0 = never (the binary walk every other kernel uses), 2 = only when the binary nodes do not fit one XCD's L2
  // (4 MiB). Bench scene: k_trace -20 % against the binary walk; instanced forest (a 2.6 MB tree): equal.
  // 3 = the 8-wide compressed form (bvh.h: Wide8Node) for host-built trees (collapsed on the host, at upload and at every
  // transforms-only update); trees it cannot take (GPU-built ones, embedded leaves) get the 4-wide form as with 1.
  int use_wide = 1;
  size_t wide_node_count = 0;
  sthip::DeviceWideScratch* wide_scratch = nullptr;  // buffers of the device-side collapse (wide.hip), kept between calls
  // sthip_scene_set_transforms (top_level.hip): the staging and scratch of the device path; whether its per-entry tables are
  // those of the resident tree; whether the host's copies of the matrices (the kept scene, top.entries[k].inv) are older
  // than the device's — a device-pointer call or a derived array left them behind (sync_kept_transforms)
  sthip::DeviceTopLevel* top_level = nullptr;
  sthip::DeviceVolumeBuild* volume_build = nullptr;  // sthip_build_volume (volume_build.hip): the build's scratch, made at first use
  bool top_level_static_valid = false;
  bool host_transforms_stale = false;
  // sthip_scene_update_vertices (refit.hip): the schedule of the resident bottom levels and the refit's scratch; what the
  // call needs to know of the uploaded arrays; whether the resident layout is one the refit serves
  sthip::DeviceRefit* refit = nullptr;
  // the distinct bottom-level roots of the resident entries and each entry's place among them (BVH_INVALID_REF: an entry
  // without a bottom level): they belong to the resident tree, as the schedule does, and are made with it
  std::vector<uint32_t> refit_roots, refit_root_of_entry;
  bool refit_roots_valid = false;
  uint32_t vertex_count = 0;
  uint64_t indices_bytes = 0;
  // sthip_scene_set_rigs / sthip_scene_animate (animate.hip): the rigs as they are resident — per rig its range of gVertices
  // and where its records start in the arrays below (rest poses and weights: one record per rigged vertex, in rig order;
  // targets: target_count x vertex_count records per rig; bones: bone_count per rig, staged on the host by every animate call)
  struct ResidentRig {
    uint32_t first = 0, count = 0, target_count = 0, bone_count = 0;
    size_t at = 0, targets_at = 0, bones_at = 0;
  };
  std::vector<ResidentRig> rigs;
  DevBuf<sthip_PackedVertexData> rig_rest, rig_targets;
  DevBuf<sthip_VertexWeight> rig_weights;
  DevBuf<sthip_TransformData> rig_bones;
  std::vector<sthip_TransformData> rig_bones_host;
  std::vector<std::array<float, 4>> rig_factors;  // of the animate call in progress
  // sthip_scene_set_environment (environment.hip): which images of gImages a material record names (their texels decided the
  // kernels: the call does not replace them), the s[y] of the rows and the rows' integrals between the passes
  std::vector<uint8_t> image_in_material;
  DevBuf<double> env_sines;
  DevBuf<float> env_integrals;
  uint32_t env_rows_per_wave = sthip::ENV_ROWS_PER_WAVE_DEFAULT;  // "env_rows_per_wave": 16 or 64 (environment.h)
  // sthip_scene_set_vertices (vertex_streams.hip): the corners of the resident meshes grouped by vertex, made at the first
  // call that asks for normals and dropped where the refit's schedule is; the staging of a call with host streams
  sthip::DeviceVertexAdjacency* adjacency = nullptr;
  DevBuf<uint8_t> stream_staging;
  // around the device work of a resident edit (device_ms of its info struct): the k_animate launches of sthip_scene_animate,
  // the enqueues of sthip_scene_set_environment, sthip_scene_set_images and sthip_scene_set_material_data
  hipEvent_t edit_ev[2] = {nullptr, nullptr};
  // sthip_scene_set_images / sthip_scene_set_material_data (image_range.hip): what the material analysis needs to run again
  // without the scene's arrays — per instance its material address and type (whatever "keep_scene" says), per image of gImages
  // the range of its level 0 as far as somebody scanned it — the alpha masks' table as uploaded, and the scan's buffers
  std::vector<sthip::MaterialInstance> material_instances;
  std::vector<sthip::ImageRange> image_ranges;
  std::vector<DeviceImage1> images1_host;
  DevBuf<uint32_t> range_partials, range_results;
  uint32_t image_range_blocks = 0;  // "image_range_blocks": 0 = from cu_count
  bool embedded_resident = false;  // the leaf triangles lie in the node array (BuiltBvh::embedded)
  bool want_wide = false;                            // the current scene is walked in its 4-wide form (decided at upload)
  bool lds_materials = true;  // k_shade stages gMaterialData in LDS when it fits 32 KB
  // frame
  DevBuf<uint8_t> views;  // gViews | gViewTransforms | gPrevViews | gPrevInverseViewTransforms
  DevBuf<float4> ray_o, ray_d, hit, beta, radiance, shadow_sum, accum, shadow_rays, light_vertices, conn, media_state, shadow_hit, shadow_ext, shadow_result;
  DevBuf<uint32_t> view_medium;
  DevBuf<uint32_t> meta, queue0, queue1, queue_kept;
  // "cull_terminal": 1 (default) = in a round where paths can reach their last vertex, k_cull_terminal hands k_shade only the
  // paths that still have something to do (kernels.h); 0 = k_shade sees the whole queue. Same frames either way.
  int cull_terminal = 1;
  DevBuf<unsigned long long> counters;
  DevBuf<float> distributions;  // gDistributions
  DevBuf<float4> presampled;    // gPresampledLights
  DevBuf<float4> bdpt;          // BDPT quantities per path (eConnectToViews)
  DevBuf<float4> rr;  // eCoherentRR: probes / group verdicts of the round in flight (FrameParams::rr)
  DevBuf<uint2> cs_nee, cs_lvc;  // eCoherentSampling: probes / group values of the round in flight (FrameParams::cs_nee, cs_lvc)
  DevBuf<float4> lvc_staging, path_contrib;  // eLVC: staged light vertices, the light paths' path_contrib (eLVCReservoirs)
  DevBuf<uint32_t> lvc_count, lvc_flags, lvc_offsets;
  DevBuf<uint8_t> lvc_tmp;
  // eNEEReservoirReuse: the append stage and its compaction, the keys / destinations of the host-side probing, the grid
  DevBuf<float4> hg_appends, hg_compact, hg_data;
  DevBuf<uint32_t> hg_count, hg_flags, hg_offsets, hg_dest, hg_checksums, hg_counters, hg_indices;
  DevBuf<uint32_t> hg_owner, hg_bucket_of, hg_append, hg_sorted_bucket, hg_sorted_append;  // scratch of the device-side grid build (hashgrid.hip)
  DevBuf<unsigned long long> hg_key64, hg_sorted_key64;
  DevBuf<uint2> hg_keys;
  DevBuf<uint8_t> hg_tmp;
  DevBuf<float4> lg_appends, lg_compact, lg_data;  // eLVCReservoirReuse: the same for gLVCHashGrid (keys / flags / tmp are shared)
  DevBuf<uint32_t> lg_checksums, lg_counters, lg_indices;
  DevBuf<uint32_t> light_trace; // gLightTraceSamples
  DevBuf<DeviceImage1> images1;  // gImage1s (alpha masks)
  DevBuf<float> image1_texels;
  DevBuf<uint8_t> image1_texels8;  // the R8 masks' texels
  DevBuf<BvhTriUv> tri_uvs;
  DevBuf<BvhTriShade> tri_shade;  // beside the leaf triangles: their vertices' normals and uvs (k_fill_tri_shade)
  DevBuf<uint32_t> hit_leaf;      // per path: the leaf triangle of its hit
  DevBuf<uint32_t> shade_stack;   // media without eDeferShadowRays: a traversal stack column per k_shade thread (visibility_walk_media)
  DevBuf<float4> debug, out_debug, shadow_debug;  // BDPTDebugMode: per-path pixel of gDebugImage, the image's staging (host pointers), the debug halves of inline shadow rays
  DevBuf<uint32_t> inst_alpha;
  DevBuf<uint8_t> inst_flags;  // per instance: INST_FLAG_* of its (untextured) material, for k_cull_terminal
  std::vector<uint8_t> inst_flags_host;
  // "answer_last_rays": 1 (default) = the last ray of a path is only queued if it can reach the bounds of an emissive instance
  // (kernels.h: aims_at_emitter); 0 = every ray is queued and traced. Same frames and ray counts either way.
  int answer_last_rays = 1;
  DevBuf<EmitterBounds> emitters;
  std::vector<EmitterBounds> emitters_host;  // the table as uploaded (sthip_scene_update_vertices makes its boxes again)
  uint32_t emitter_count = 0;  // 0: not applicable to this scene (no or too many emissive triangle instances)
  DevBuf<unsigned long long> qctl;  // queue control lines (queue_ctl)
  DevBuf<uint32_t> post_scratch;  // maxima / metric accumulator of post.h
  DevBuf<float4> denoise_guide;   // sthip_denoise_filter: {n.x, n.y, n.z, z} per pixel, grows with the largest extent seen
  uint32_t denoise_block = 0;     // "denoise_block": 0 = 32x8 lanes per block, 1 = 16x16
  DevBuf<sthip_ray> ray_staging;  // sthip_trace_rays with host pointers
  DevBuf<sthip_hit> hit_staging;
  DevBuf<float4> out_radiance, out_albedo;  // staging of the colour images (out_debug too): color_bytes() per entry, so 16 B entries hold 1 or 2
  DevBuf<float4> albedo_stage;  // half colour precision: k_shade's binary32 albedo, which k_resolve rounds into the RGBA16F image
  // "half_color_precision": the colour images of sthip_render and of the post calls are RGBA16F (8 B per pixel) instead of RGBA32F
  bool half_color = false;
  size_t color_bytes() const { return half_color ? 8 : 16; }
  DevBuf<sthip_VisibilityInfo> out_visibility;
  DevBuf<sthip_DepthInfo> out_depth;
  DevBuf<float2> out_prev_uv;
  uint32_t shard_rank = 0, shard_count = 1, tile_w = 64, tile_h = 32;
  // options / stats
  bool count_traversal = false, time_kernels = false;
  bool hashgrid_serial = false;  // "hashgrid_serial": build the reuse grids with the one-thread probe sequence (hashgrid.hip's rare-case path; tests)
  // "reuse_grids_persist": the grids the LAST seed of a call leaves are what the FIRST seed of the next call looks into — upstream's
  // previous frame for a host that renders one frame per call (BDPT.cpp:482-483,621-627). The key says what they were built for.
  bool reuse_persist = false, reuse_grids_valid = false;
  uint64_t reuse_key[3] = {0, 0, 0};
  uint32_t refill_idle = 16, inner_min_lanes = 24, trace_blocks_per_cu = 0;
  uint64_t max_paths_in_flight = 1ull << 22;  // (sthip_create sizes it to the device: 2^26 on a 288 GB MI355X — launches large enough that their
                                              // tails stop mattering: atrium x 8 seeds +7 %, forest at 4K x 16 +38 % over 2^22; tools/in_flight_sweep.py)
  bool packet_primary = true;  // the first bounce is traced as wave packets (k_trace_primary)
  // "reuse_first_hits" (first_hits.h): the hits of the first bounce do not depend on the seed, so the packet kernel's output
  // for ONE seed's paths is kept here (20 B per path, allocated at first use; a call renders without them if that fails) and
  // the kernel runs again only when the key of a call differs from the key they were traced for. `scene_serial` counts the
  // calls that can move a triangle, an instance or an alpha mask. The pair (valid, key) changes only where the launch that
  // fills the buffers is enqueued (run_batches: past the point where a render is tried again), or where the hits are dropped.
  bool reuse_first_hits = true, first_hits_valid = false;
  uint64_t scene_serial = 0;
  sthip::FirstHitKey first_hit_key{};
  DevBuf<float4> first_hit;
  DevBuf<uint32_t> first_hit_leaf;
  bool fuse_trace = true;  // closest-hit rays of a bounce and the shadow rays of the previous one in one launch
  int bvh_builder = 0;  // sthip::BvhBuilderKind
  uint32_t sah_top_size = 64;  // "sah_top" (measured 32 .. 16384: 64 traces fastest): the GPU builder's subtrees of at most this many triangles get a host-built SAH top (0: off)
  int lbvh_algorithm = 1, ploc_radius = 4;  // of the GPU builder (bvh_build.h: DeviceBuildTarget); radius measured: 4 traces fastest (2 .. 32 tried)
  // levels of the per-lane LDS traversal stack at most; a higher tree runs the BOUNDED instantiations (traverse.h) with the
  // full stack of an overflowing ray in global memory (spill)
  // measured (atrium, PLOC tree 40 high): the bounded instantiation costs ~2.5 % per step, a fourth resident block is worth
  // ~13 %, a treetop ~3 %: so the whole stack stays in LDS as long as four blocks of it fit (40 levels = 160 KB per CU)
  uint32_t lds_stack_threshold = 40, lds_stack_cap = 32;
  DevBuf<uint32_t> spill;
  DevBuf<float4> deep_rays;  // rays that overflowed a bounded LDS stack (k_trace_deep), and their count
  DevBuf<uint32_t> deep_count;
  sthip_stats stats{};
  hipError_t last_hip_error = hipSuccess;  // of the last failed HIP_TRY (sthip_render halves its batch after an out-of-memory)
  bool render_launched = false;            // the render call in progress has enqueued work (no second attempt from here on)
  bool stats_pending = false;  // ray / traversal counters of the last render still live on the device
  hipEvent_t ev[2] = {nullptr, nullptr};
  // sthip_render_async: "output_ring" staging sets (made at the first submit), the copy stream, tickets issued / retired
  uint32_t output_ring = 2;
  std::vector<AsyncSlot*> ring;
  hipStream_t copy_stream = nullptr;
  uint64_t next_ticket = 1, retired = 0;
  // a finished frame whose slot a later submit took over before its ticket was waited for: its counters and the caller's gRayCount
  struct FinishedFrame {
    std::vector<unsigned long long> counters;
    uint64_t* ray_count = nullptr;
  };
  std::map<uint64_t, FinishedFrame> finished;
  std::vector<void*> host_allocs;  // sthip_host_alloc
};

// The traversal stack is stack_depth x 1 KB of dynamic LDS per 256-thread block. Up to 64 KB needs nothing; beyond it
// (deep LBVH trees of clustered scenes) the kernels must be told (hipFuncAttributeMaxDynamicSharedMemorySize), and the
// CU holds fewer blocks. 152 KB leaves room for the runtime's own LDS use.
#define STHIP_MAX_STACK_LDS ((size_t)152 * 1024)
// Trees higher than the LDS cap (lds_stack_levels) keep only that many levels in LDS; the rare ray that needs more is traced
// again with a global-memory stack of the tree's full height — bounded here so that the spill buffer stays small
#define STHIP_MAX_STACK_DEPTH 512u

#define HIP_TRY(ctx, expr)                                                                            \
  do {                                                                                                \
    hipError_t _e = (expr);                                                                           \
    if (_e != hipSuccess) {                                                                           \
      (ctx)->error = std::string(#expr) + ": " + hipGetErrorString(_e);                               \
      (ctx)->last_hip_error = _e;                                                                     \
      return STHIP_ERR_HIP;                                                                           \
    }                                                                                                 \
  } while (0)

inline int fail(sthip_ctx* ctx, int code, const std::string& msg) {
  ctx->error = msg;
  return code;
}

// post.hip: the dense half of sthip_build_volume, shared with sthip_scene_set_volume (api.hip)
int dense_volume_scan(sthip_ctx* ctx, const char* call, const sthip_dense_volume_desc* d, DevBuf<float>& staged, sthip::VolumeBuildInput& in, sthip::VolumeBuildCounts& c, sthip::VolumeHeader& header,
                      sthip_volume_info* info, float& scan_ms);

#pragma GCC visibility pop
