// api.hip — the C ABI of include/sthip.h: context, scene upload, the edits of a resident scene, the per-frame launch sequence
// (the calls after the path and the ceilings: post.hip; the context struct both units share: context.h). The one unit that
// compiles and launches the kernels of kernels.h.
//
// sthip_render is the replacement of the dispatch sequence BDPT::render records
// (src/Node/BDPT.cpp:607-720: fill gShadowRays, dispatch sample_visibility, barrier, dispatch
// trace_shadows) and of the running-mean accumulation the denoiser applies with default settings
// (src/Node/Denoiser.cpp:73,186-213). There is no CPU fallback: every entry point needs a HIP device.
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
#include "animate.h"
#include "environment.h"
#include "bvh_build.h"
#include "first_hits.h"
#include "image_range.h"
#include "kernel_instances.h"  // kernels.h + the instantiations that live in shade_*.hip / trace_kernels.hip
#include "mips.h"
#include "scene_prepare.h"
#include "top_level.h"
#include "context.h"

STHIP_DECLARE_KERNEL_INSTANCES

namespace sthip {
hipError_t lvc_compact(const float4* staging, uint32_t slots_per_seed, uint32_t seeds, uint32_t vertices_per_seed, float4* cache, uint32_t* counts, uint32_t* flags, uint32_t* offsets,
                       void* tmp, size_t& tmp_bytes, hipStream_t stream, uint32_t rec = 4, uint32_t flag_at = 2);  // lvc.hip
hipError_t hashgrid_build_device(const uint2* keys, const uint32_t* count, uint32_t slots, uint32_t buckets, uint32_t* checksums, uint32_t* counters, uint32_t* indices, uint32_t* dest, uint32_t* owner,
                                 uint32_t* bucket_of, uint32_t* append_index, uint32_t* sorted_bucket, uint32_t* sorted_append, unsigned long long* key64, unsigned long long* sorted_key64, void* tmp,
                                 size_t& tmp_bytes, hipStream_t stream, bool force_serial = false);  // hashgrid.hip
}

static thread_local std::string g_create_error;

// The instantiations that exist, by key (kernel_variants.h): made from the lists the definitions are compiled from, so that a
// variant outside them has no entry here — a lookup that finds none is the caller's error, not an instantiation in this file
struct KernelEntry {
  uint32_t key;
  const void* fn;
};
#define STHIP_SHADE_ENTRY(T, E, L, M, P, D) {sthip::shade_key(T, E, L, M, P, D), (const void*)&k_shade<T, E, L, M, P, D>},
#define STHIP_TRACE_ENTRY(C, A, B, T, W) {sthip::trace_key(C, A, B, T, W), (const void*)&k_trace<C, A, B, T, W>},
#define STHIP_LIGHT_ENTRY(T, E, M) {sthip::shade_light_key(T, E, M), (const void*)&k_shade_light<T, E, M>},
static const KernelEntry g_shade_kernels[] = {STHIP_SHADE_ALL(STHIP_SHADE_ENTRY)};
static const KernelEntry g_trace_kernels[] = {STHIP_TRACE_ALL(STHIP_TRACE_ENTRY)};
static const KernelEntry g_shade_light_kernels[] = {STHIP_SHADE_LIGHT(STHIP_LIGHT_ENTRY)};

template <size_t N>
static const void* find_kernel(const KernelEntry (&table)[N], uint32_t key) {
  for (const KernelEntry& e : table)
    if (e.key == key) return e.fn;
  return nullptr;
}
// k_trace by (count_traversal, alpha masks / volumes, bounded stack) for the tree the scene is walked in: the 8-wide or 4-wide
// form ("wide_bvh"; never with the treetop) or the binary one; the 4-wide form over its leaf records where the tree has them
// ("leaf_pairs") and the instantiation exists
static const void* trace_kernel(const DeviceBvh& bvh, bool count, bool alpha, bool top) {
  const int wide = bvh.wide8_nodes ? 2 : bvh.wide_nodes ? (bvh.pairs && !alpha ? 3 : 1) : 0;
  return find_kernel(g_trace_kernels, sthip::trace_key(count, alpha, bvh.spill != nullptr, top && wide == 0, wide));
}
// The kernels with two bool template arguments, all four instantiations of each compiled here
#define STHIP_KERNEL2(K, a, b) ((a) ? ((b) ? (const void*)&K<true, true> : (const void*)&K<true, false>) : ((b) ? (const void*)&K<false, true> : (const void*)&K<false, false>))

// One launch of a kernel that was picked at run time; `args` are the kernel's parameters, of exactly their types
template <typename... A>
static void launch_kernel(const void* fn, uint32_t grid, size_t lds, hipStream_t st, const A&... args) {
  void* ptrs[] = {(void*)&args...};
  (void)hipLaunchKernel(fn, dim3(grid), dim3(STHIP_BLOCK), ptrs, lds, st);
}


static void fill_counter_stats(sthip_ctx* ctx, const unsigned long long* c) {
  ctx->stats.rays_total = c[CNT_RAYS_CLOSEST] + c[CNT_RAYS_SHADOW];
  ctx->stats.rays_path = c[CNT_RAYS_CLOSEST] - c[CNT_CROSSINGS];
  ctx->stats.rays_shadow = c[CNT_RAYS_SHADOW];
  ctx->stats.nodes_visited = c[CNT_NODES];
  ctx->stats.tris_tested = c[CNT_TRIS];
  ctx->stats.nodes_visited_shadow = c[CNT_NODES + 1];
  ctx->stats.tris_tested_shadow = c[CNT_TRIS + 1];
  for (int k = 0; k < 2; k++) {
    ctx->stats.inner_slots[k] = c[CNT_INNER_SLOTS + k];
    ctx->stats.tri_slots[k] = c[CNT_TRI_SLOTS + k];
    ctx->stats.round_slots[k] = c[CNT_ROUND_SLOTS + k];
    ctx->stats.busy_rounds[k] = c[CNT_BUSY_ROUNDS + k];
  }
  for (int k = 0; k < 8; k++) ctx->stats.lane_states[k] = c[CNT_LANE_STATES + k];
  ctx->stats.rays_answered = c[CNT_RAYS_ANSWERED];
  ctx->stats.nodes_visited_primary = c[CNT_NODES_PRIMARY];
  ctx->stats.tris_tested_primary = c[CNT_TRIS_PRIMARY];
}

static uint32_t grid_for(const sthip_ctx* ctx, size_t n);
static void bind_leaf_pairs(sthip_ctx* ctx);


// ---- frames in flight of sthip_render_async ----
static AsyncSlot* slot_of(sthip_ctx* ctx, uint64_t ticket) { return ctx->ring[ticket % ctx->ring.size()]; }

// Tickets retired + 1 .. t, in order; their "copied" events have been reached (the copy stream runs them in submission order,
// so the caller has waited for t's). What the host owes a finished frame: gRayCount and the stats, from the pinned record.
static void retire_through(sthip_ctx* ctx, uint64_t t) {
  while (ctx->retired < t) {
    const uint64_t k = ++ctx->retired;
    AsyncSlot* s = slot_of(ctx, k);
    const unsigned long long* c = nullptr;
    uint64_t* ray_count = nullptr;
    const auto it = ctx->finished.find(k);
    if (s->ticket == k) {
      c = s->record;
      ray_count = s->ray_count;
    } else if (it != ctx->finished.end()) {
      c = it->second.counters.data();
      ray_count = it->second.ray_count;
    } else {
      continue;
    }
    if (ray_count) {
      ray_count[0] = c[CNT_RAYS_CLOSEST] + c[CNT_RAYS_SHADOW];
      ray_count[1] = c[CNT_RAYS_CLOSEST] - c[CNT_CROSSINGS];
    }
    fill_counter_stats(ctx, c);
    ctx->stats_pending = false;
    if (s->ticket == k) {
      s->ticket = 0;
      s->ray_count = nullptr;
    } else {
      ctx->finished.erase(it);
    }
  }
}

// Blocks until ticket t's outputs are in host memory (and with them every earlier ticket's: the copy stream runs the frames in
// submission order). A ticket that is no longer in its slot was completed when a later submit took the slot over.
static hipError_t complete_ticket(sthip_ctx* ctx, uint64_t t) {
  AsyncSlot* s = slot_of(ctx, t);
  return s->ticket == t ? hipEventSynchronize(s->copied) : hipSuccess;
}

// Completes every frame in flight (render and copy) and retires its ticket; the tickets stay waitable.
static hipError_t drain_in_flight(sthip_ctx* ctx) {
  if (ctx->retired + 1 == ctx->next_ticket) return hipSuccess;
  const hipError_t e = complete_ticket(ctx, ctx->next_ticket - 1);
  if (e != hipSuccess) return e;
  retire_through(ctx, ctx->next_ticket - 1);
  return hipSuccess;
}

static void release_ring(sthip_ctx* ctx) {
  for (AsyncSlot* s : ctx->ring) delete s;
  ctx->ring.clear();
}

// Nothing is in flight any more: the caller's stream has been waited for, and the frames of sthip_render_async are complete.
// What a call does before it writes what frames in flight still read.
static int quiesce(sthip_ctx* ctx) {
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, drain_in_flight(ctx));
  return STHIP_OK;
}

// ---- the steps the edit calls share ----
// The two events around the device work of an edit, made at first use
static int make_edit_events(sthip_ctx* ctx) {
  for (int k = 0; k < 2; k++)
    if (!ctx->edit_ev[k]) HIP_TRY(ctx, hipEventCreate(&ctx->edit_ev[k]));
  return STHIP_OK;
}
// device_ms between the two events (the stream has been waited for) and total_ms since the call began
template <typename Info>
static void fill_edit_times(sthip_ctx* ctx, Info* info, std::chrono::steady_clock::time_point t0) {
  info->device_ms = 0;
  (void)hipEventElapsedTime(&info->device_ms, ctx->edit_ev[0], ctx->edit_ev[1]);
  info->total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// `bytes` of gMaterialData from `offset` on: the host mirror, the device array (in stream order) and the kept scene
static int write_material_bytes(sthip_ctx* ctx, size_t offset, const void* data, size_t bytes, hipStream_t st) {
  memcpy(ctx->materials_host.data() + offset, data, bytes);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->materials.p + offset, ctx->materials_host.data() + offset, bytes, hipMemcpyHostToDevice, st));
  if (ctx->kept.valid && ctx->kept.materials.size() == ctx->materials_host.size()) memcpy(ctx->kept.materials.data() + offset, data, bytes);
  return STHIP_OK;
}

// Level 0 of gImages[index] (`mask`: of gImage1s[index]) from `pixels`, host or device memory, in the format the image is resident in
static int copy_image_level0(sthip_ctx* ctx, bool mask, uint32_t index, const void* pixels, bool device_ptr, hipStream_t st) {
  const hipMemcpyKind kind = device_ptr ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  if (mask) {
    const DeviceImage1& im = ctx->images1_host[index];
    const size_t texels = (size_t)im.w * im.h;
    if (im.format == STHIP_IMAGE_FORMAT_R8_UNORM)
      HIP_TRY(ctx, hipMemcpyAsync(ctx->image1_texels8.p + im.offset, pixels, texels, kind, st));
    else
      HIP_TRY(ctx, hipMemcpyAsync(ctx->image1_texels.p + im.offset, pixels, texels * 4, kind, st));
    return STHIP_OK;
  }
  const DeviceImage& im = ctx->images_host[index];
  const size_t texels = (size_t)im.w[0] * im.h[0];
  if (im.format == STHIP_IMAGE_FORMAT_RGBA8_UNORM)
    HIP_TRY(ctx, hipMemcpyAsync(ctx->image_texels8.p + im.offset[0], pixels, texels * 4, kind, st));
  else
    HIP_TRY(ctx, hipMemcpyAsync(ctx->image_texels.p + im.offset[0], pixels, texels * 16, kind, st));
  return STHIP_OK;
}
// ... and the levels above it, each one launch over the level before it (mips.hip)
static int rebuild_image_mips(sthip_ctx* ctx, uint32_t index, hipStream_t st, const char* call) {
  const DeviceImage& im = ctx->images_host[index];
  const bool rgba8 = im.format == STHIP_IMAGE_FORMAT_RGBA8_UNORM;
  std::string err;
  for (uint32_t level = 0; level + 1 < im.levels; level++) {
    const bool ok = rgba8 ? sthip::mip_rgba8_launch(ctx->image_texels8.p + im.offset[level], im.w[level], im.h[level], ctx->image_texels8.p + im.offset[level + 1], ctx->cu_count, st, err)
                          : sthip::mip_rgba32f_launch(ctx->image_texels.p + im.offset[level], im.w[level], im.h[level], ctx->image_texels.p + im.offset[level + 1], ctx->cu_count, st, err);
    if (!ok) return fail(ctx, STHIP_ERR_HIP, std::string(call) + ": " + err);
  }
  return STHIP_OK;
}
// The kept copy of that image follows: host pixels are copied and the copy is current; device pixels leave it stale
// (sync_kept_environment fetches them before anything is built from the kept scene)
static void kept_image_follows(sthip_ctx* ctx, bool mask, uint32_t index, const void* pixels, bool device_ptr) {
  if (!ctx->kept.valid) return;
  std::vector<std::vector<float>>& floats = mask ? ctx->kept.image1_pixels : ctx->kept.image_pixels;
  std::vector<std::vector<uint8_t>>& bytes = mask ? ctx->kept.image1_bytes : ctx->kept.image_bytes;
  std::set<uint32_t>& stale = mask ? ctx->kept.stale_images1 : ctx->kept.stale_images;
  if (index >= floats.size() || index >= bytes.size()) return;
  if (device_ptr) {
    stale.insert(index);
    return;
  }
  const size_t values = mask ? (size_t)ctx->images1_host[index].w * ctx->images1_host[index].h : (size_t)ctx->images_host[index].w[0] * ctx->images_host[index].h[0] * 4;
  if (bytes[index].size() == values) memcpy(bytes[index].data(), pixels, values);
  if (floats[index].size() == values) memcpy(floats[index].data(), pixels, values * 4);
  stale.erase(index);
}

// Measurement only (sthip.h; tools/environment_times.py, tools/material_update_times.py): HIP events at the borders of a call's
// stages, and one JSON line per call appended to the file an environment variable names. The variable is read once per
// process (each variable has its accessor, all of one shape); without it no event is made and no file touched.
static const char* times_file(const char* variable) {
  const char* v = getenv(variable);
  return v && *v ? v : nullptr;
}
static const char* environment_times_file() {  // STHIP_ENVIRONMENT_TIMES=<file>: one line per table-building call with the HIP-event time of each stage
  static const char* const path = times_file("STHIP_ENVIRONMENT_TIMES");
  return path;
}
static const char* vertex_times_file() {  // STHIP_VERTEX_TIMES=<file>: one line per sthip_scene_set_vertices call with the HIP-event time of each of its kernels
  static const char* const path = times_file("STHIP_VERTEX_TIMES");
  return path;
}
struct StageTimer {
  enum { MAX_EVENTS = 8 };
  hipEvent_t ev[MAX_EVENTS] = {};  // ev[k]: recorded when stage k is enqueued (a stage the call skips is recorded where it would stand: 0 ms)
  const char* path;
  int events;
  bool on = false;
  StageTimer(const char* path, bool wanted, int events) : path(path), events(events) {
    if (!path || !wanted || events > MAX_EVENTS) return;
    on = true;  // (a failure to make an event only loses the measurement)
    for (int k = 0; k < events; k++) on = on && hipEventCreate(&ev[k]) == hipSuccess;
  }
  StageTimer(const StageTimer&) = delete;
  ~StageTimer() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  void mark(int k, hipStream_t st) {
    if (on) (void)hipEventRecord(ev[k], st);
  }
  // after the stream has been waited for: {<head>, "<names[k]>": <ms from event k to event k + 1>, ...}
  void write(const std::string& head, const char* const* names) {
    if (!on) return;
    if (FILE* f = fopen(path, "a")) {
      fprintf(f, "{%s", head.c_str());
      for (int k = 0; k + 1 < events; k++) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ev[k], ev[k + 1]);
        fprintf(f, ", \"%s\": %.5f", names[k], ms);
      }
      fprintf(f, "}\n");
      fclose(f);
    }
  }
};

extern "C" {

int sthip_abi_version(void) { return STHIP_ABI_VERSION; }

int sthip_create(int device, sthip_ctx** out_ctx) {
  if (!out_ctx) {
    g_create_error = "out_ctx is NULL";
    return STHIP_ERR_INVALID_ARGUMENT;
  }
  *out_ctx = nullptr;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count == 0) {
    g_create_error = std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0") +
                     " (libstratum_hip has no CPU backend)";
    return STHIP_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= count) {
    g_create_error = "device index out of range";
    return STHIP_ERR_INVALID_ARGUMENT;
  }
  e = hipSetDevice(device);
  if (e != hipSuccess) {
    g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e);
    return STHIP_ERR_HIP;
  }
  sthip_ctx* ctx = new sthip_ctx();
  ctx->device = device;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
    ctx->cu_count = prop.multiProcessorCount;
    // paths in flight by default: the largest power of two that leaves 4 KB of device memory per path (a path costs ~330 B of
    // state, queues and shadow records at the default flags, more with light subpaths): 2^26 on a 288 GB MI355X
    // — of the memory that is FREE now: a host application (or other contexts on the device) may hold most of it; should the
    // batch still not fit when a render allocates it, sthip_render halves it and tries again
    size_t free_bytes = 0, total_bytes = 0;
    if (hipMemGetInfo(&free_bytes, &total_bytes) != hipSuccess) free_bytes = prop.totalGlobalMem;
    uint64_t paths = 1ull << 18;
    while (paths * 2 * 4096 <= (uint64_t)free_bytes && paths < (1ull << 27)) paths *= 2;
    ctx->max_paths_in_flight = paths;
  }
  (void)hipEventCreate(&ctx->ev[0]);
  (void)hipEventCreate(&ctx->ev[1]);
  {  // dynamic LDS beyond the 64 KB default for the kernels that carry the traversal stack
    const int lds_max = 160 * 1024;
    for (const KernelEntry& e : g_trace_kernels) (void)hipFuncSetAttribute(e.fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    for (int k = 0; k < 4; k++) (void)hipFuncSetAttribute(STHIP_KERNEL2(k_trace_batch, (k & 2) != 0, (k & 1) != 0), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
  }
  ctx->stats.bvh_node_bytes = sizeof(BvhNodePacked);
  ctx->stats.bvh_tri_bytes = sizeof(BvhTri);
  *out_ctx = ctx;
  return STHIP_OK;
}

void sthip_destroy(sthip_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  if (ctx->retired + 1 != ctx->next_ticket) retire_through(ctx, ctx->next_ticket - 1);  // (the device is idle: every copy has landed)
  release_ring(ctx);
  if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
  for (void* q : ctx->host_allocs) (void)hipHostFree(q);
  sthip::device_wide_scratch_destroy(ctx->wide_scratch);
  ctx->wide_scratch = nullptr;
  sthip::device_top_level_destroy(ctx->top_level);
  ctx->top_level = nullptr;
  sthip::device_volume_build_destroy(ctx->volume_build);
  ctx->volume_build = nullptr;
  sthip::device_refit_destroy(ctx->refit);
  ctx->refit = nullptr;
  sthip::device_vertex_adjacency_destroy(ctx->adjacency);
  ctx->adjacency = nullptr;
  for (int k = 0; k < 2; k++)
    if (ctx->edit_ev[k]) (void)hipEventDestroy(ctx->edit_ev[k]);
  ctx->vertices.release();
  ctx->volume_words.release();
  ctx->volumes.release();
  ctx->indices.release();
  ctx->instances.release();
  ctx->xf.release();
  ctx->inv_xf.release();
  ctx->motion_xf.release();
  ctx->materials.release();
  ctx->lights.release();
  ctx->images.release();
  ctx->image_texels.release();
  ctx->image_texels8.release();
  ctx->cone.release();
  ctx->nodes.release();
  ctx->tris.release();
  ctx->entries.release();
  ctx->views.release();
  ctx->ray_o.release();
  ctx->ray_d.release();
  ctx->hit.release();
  ctx->hit_leaf.release();
  ctx->first_hit.release();
  ctx->first_hit_leaf.release();
  ctx->debug.release();
  ctx->shadow_debug.release();
  ctx->beta.release();
  ctx->radiance.release();
  ctx->shadow_sum.release();
  ctx->accum.release();
  ctx->shadow_rays.release();
  ctx->light_vertices.release();
  ctx->media_state.release();
  ctx->shade_stack.release();
  ctx->shadow_hit.release();
  ctx->shadow_ext.release();
  ctx->shadow_result.release();
  ctx->view_medium.release();
  ctx->conn.release();
  ctx->meta.release();
  ctx->queue0.release();
  ctx->queue1.release();
  ctx->counters.release();
  ctx->distributions.release();
  ctx->presampled.release();
  ctx->bdpt.release();
  ctx->light_trace.release();
  ctx->images1.release();
  ctx->image1_texels.release();
  ctx->image1_texels8.release();
  ctx->tri_uvs.release();
  ctx->tri_shade.release();
  ctx->hit_leaf.release();
  ctx->inst_alpha.release();
  ctx->inst_flags.release();
  ctx->qctl.release();
  ctx->post_scratch.release();
  ctx->out_radiance.release();
  ctx->out_albedo.release();
  ctx->albedo_stage.release();
  ctx->out_visibility.release();
  ctx->out_depth.release();
  ctx->out_prev_uv.release();
  if (ctx->ev[0]) (void)hipEventDestroy(ctx->ev[0]);
  if (ctx->ev[1]) (void)hipEventDestroy(ctx->ev[1]);
  delete ctx;
}

const char* sthip_last_error(const sthip_ctx* ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }

int sthip_set_stream(sthip_ctx* ctx, void* hip_stream) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  if ((hipStream_t)hip_stream != ctx->stream && ctx->retired + 1 != ctx->next_ticket) {  // frames of sthip_render_async in flight are ordered by the stream they were enqueued on: a CHANGE of stream completes them
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, drain_in_flight(ctx));
  }
  if ((hipStream_t)hip_stream != ctx->stream) ctx->first_hits_valid = false;  // (nothing orders the new stream behind the launch that filled them)
  ctx->stream = (hipStream_t)hip_stream;
  return STHIP_OK;
}

int sthip_set_shard(sthip_ctx* ctx, uint32_t shard_rank, uint32_t shard_count, uint32_t tile_w, uint32_t tile_h) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  if (shard_count == 0 || shard_rank >= shard_count || tile_w == 0 || tile_h == 0 || (tile_w & 7u) || (tile_h & 7u))
    return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "shard: need rank < count and tile sizes that are multiples of 8");
  ctx->shard_rank = shard_rank;
  ctx->shard_count = shard_count;
  ctx->tile_w = tile_w;
  ctx->tile_h = tile_h;
  ctx->first_hits_valid = false;
  return STHIP_OK;
}

int sthip_set_option(sthip_ctx* ctx, const char* name, int64_t value) {
  if (!ctx || !name) return STHIP_ERR_INVALID_ARGUMENT;
  if (!strcmp(name, "count_traversal"))
    ctx->count_traversal = value != 0;
  else if (!strcmp(name, "time_kernels"))
    ctx->time_kernels = value != 0;
  else if (!strcmp(name, "fuse_trace"))
    ctx->fuse_trace = value != 0;
  else if (!strcmp(name, "packet_primary"))
    ctx->packet_primary = value != 0;
  else if (!strcmp(name, "answer_last_rays"))
    ctx->answer_last_rays = value != 0;
  else if (!strcmp(name, "reuse_first_hits")) {  // setting it (to either value) also drops the hits kept so far
    ctx->reuse_first_hits = value != 0;
    ctx->first_hits_valid = false;
  }
  else if (!strcmp(name, "cull_terminal"))
    ctx->cull_terminal = value != 0;
  else if (!strcmp(name, "refill_idle"))
    ctx->refill_idle = (uint32_t)std::min<int64_t>(64, std::max<int64_t>(1, value));
  else if (!strcmp(name, "bvh_builder"))
    ctx->bvh_builder = value == 1 ? 1 : 0;
  else if (!strcmp(name, "lds_materials"))
    ctx->lds_materials = value != 0;
  else if (!strcmp(name, "embed_leaves"))  // takes effect at the next sthip_scene_upload
    ctx->embed_leaves = value != 0;
  else if (!strcmp(name, "keep_scene")) {  // takes effect at the next sthip_scene_upload
    ctx->keep_scene = value != 0;
    if (!ctx->keep_scene) ctx->kept = KeptScene();
  } else if (!strcmp(name, "wide_bvh"))  // takes effect at the next sthip_scene_upload (host-built trees only)
    ctx->use_wide = (int)std::min<int64_t>(std::max<int64_t>(value, 0), 3);
  else if (!strcmp(name, "poison_deep_queue")) {  // tests: leaves the deep queue's control words as a call cut short between k_trace and k_trace_deep would (the next render must not care)
    if (value && ctx->deep_count.p) {
      const uint32_t junk[2] = {5u, 3u};
      (void)hipSetDevice(ctx->device);
      (void)hipStreamSynchronize(ctx->stream);
      if (hipMemcpy(ctx->deep_count.p, junk, 8, hipMemcpyHostToDevice) != hipSuccess) return fail(ctx, STHIP_ERR_HIP, "poison_deep_queue: copy failed");
    }
  } else if (!strcmp(name, "leaf_pairs")) {  // takes effect at the next render: the same tree, its leaves from the records or from BvhTri
    ctx->leaf_pairs = value != 0;
    bind_leaf_pairs(ctx);
  } else if (!strcmp(name, "tri_min_lanes"))  // the 8-wide walk's leaf phase goes on while at least this many lanes hold a triangle
    ctx->tri_min_lanes = ctx->bvh.wide8_tri_min = (uint32_t)std::min<int64_t>(std::max<int64_t>(value, 1), 64);
  else if (!strcmp(name, "lbvh_algorithm"))  // 0: Karras radix tree, 1: PLOC (default)
    ctx->lbvh_algorithm = value == 0 ? 0 : 1;
  else if (!strcmp(name, "lds_stack_levels")) {  // takes effect at the next sthip_scene_upload / sthip_scene_update_transforms
    ctx->lds_stack_cap = ctx->lds_stack_threshold = (uint32_t)std::min<int64_t>(std::max<int64_t>(value, 4), 150);
  } else if (!strcmp(name, "ploc_radius"))
    ctx->ploc_radius = (int)std::min<int64_t>(std::max<int64_t>(value, 1), 32);
  else if (!strcmp(name, "sah_top"))
    ctx->sah_top_size = value <= 0 ? 0u : (uint32_t)std::min<int64_t>(std::max<int64_t>(value, 16), 1 << 20);  // (the reserved host-node room covers frontiers down to 16)
  else if (!strcmp(name, "max_paths_in_flight"))
    ctx->max_paths_in_flight = (uint64_t)std::max<int64_t>(1, value);
  else if (!strcmp(name, "trace_blocks_per_cu"))
    ctx->trace_blocks_per_cu = (uint32_t)std::min<int64_t>(16, std::max<int64_t>(0, value));
  else if (!strcmp(name, "treetop"))  // takes effect at the next sthip_scene_upload / sthip_scene_update_transforms
    ctx->use_treetop = value != 0;
  else if (!strcmp(name, "hashgrid_serial"))
    ctx->hashgrid_serial = value != 0;
  else if (!strcmp(name, "reuse_grids_persist")) {  // setting it (to either value) also drops the grids kept so far
    ctx->reuse_persist = value != 0;
    ctx->reuse_grids_valid = false;
  }
  else if (!strcmp(name, "half_color_precision")) {  // takes effect at the next call; refused outside 0 / 1
    if (value != 0 && value != 1) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "half_color_precision: 0 or 1");
    ctx->half_color = value != 0;
  } else if (!strcmp(name, "output_ring")) {  // frames in flight of sthip_render_async = device staging sets; a change first completes the frames in flight
    if (value < 1 || value > 8) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "output_ring: 1 .. 8");
    if ((uint32_t)value != ctx->output_ring) {
      HIP_TRY(ctx, hipSetDevice(ctx->device));
      HIP_TRY(ctx, drain_in_flight(ctx));
      release_ring(ctx);
      ctx->output_ring = (uint32_t)value;
    }
  } else if (!strcmp(name, "denoise_block")) {
    if (value != 0 && value != 1) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "denoise_block: 0 (32x8) or 1 (16x16)");
    ctx->denoise_block = (uint32_t)value;
  } else if (!strcmp(name, "env_rows_per_wave")) {  // rows a wave of k_env_rows owns (environment.h)
    if (value != 16 && value != 64) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "env_rows_per_wave: 16 or 64");
    ctx->env_rows_per_wave = (uint32_t)value;
  } else if (!strcmp(name, "image_range_blocks")) {  // blocks of k_image_range (image_range.h); 0 = sized from the CU count
    if (value < 0 || value > (int64_t)sthip::IMAGE_RANGE_MAX_BLOCKS) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "image_range_blocks: 0 (default) or 1 .. 65535");
    ctx->image_range_blocks = (uint32_t)value;
  } else if (!strcmp(name, "inner_min_lanes"))
    ctx->inner_min_lanes = (uint32_t)std::min<int64_t>(64, std::max<int64_t>(1, value));
  else
    return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, std::string("unknown option ") + name);
  return STHIP_OK;
}

int sthip_get_stats(sthip_ctx* ctx, sthip_stats* out) {
  if (!ctx || !out) return STHIP_ERR_INVALID_ARGUMENT;
  if (ctx->stats_pending) {
    unsigned long long c[CNT_TOTAL];
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(c, ctx->counters.p, sizeof(c), hipMemcpyDeviceToHost));
    fill_counter_stats(ctx, c);
    ctx->stats_pending = false;
  }
  *out = ctx->stats;
  out->bvh_node_bytes = ctx->bvh.wide8_nodes ? (uint32_t)sizeof(Wide8Node) : ctx->bvh.wide_nodes ? (uint32_t)sizeof(WideNode) : (uint32_t)sizeof(BvhNodePacked);  // of the nodes k_trace walks (its visits are what the counters count)
  out->bvh_tri_bytes = sizeof(BvhTri);
  out->bvh_nodes = ctx->bvh_nodes;
  out->bvh_tris = ctx->bvh_tris;
  return STHIP_OK;
}

static size_t stack_bytes(const sthip_ctx* ctx);
static size_t trace_lds_bytes(const sthip_ctx* ctx);
static int trace_occupancy(const sthip_ctx* ctx, size_t lds_bytes);
static int configure_stack(sthip_ctx* ctx);
static int refresh_treetop(sthip_ctx* ctx);
static int sync_kept_transforms(sthip_ctx* ctx);
static int sync_kept_volumes(sthip_ctx* ctx);
// packs `count` nodes and writes them into the node array from slot `first` on
static hipError_t upload_nodes(sthip_ctx* ctx, size_t first, const BvhNode* nodes, size_t count) {
  std::vector<BvhNodePacked> packed;
  sthip::pack_nodes(nodes, count, packed);
  std::vector<BvhNodeSlot> slots(count);
  memset(slots.data(), 0, count * sizeof(BvhNodeSlot));
  for (size_t i = 0; i < count; i++) slots[i].n = packed[i];
  return hipMemcpy(ctx->nodes.p + first, slots.data(), count * sizeof(BvhNodeSlot), hipMemcpyHostToDevice);
}

// the leaf records k_trace reads: the resident ones while "leaf_pairs" is on
static void bind_leaf_pairs(sthip_ctx* ctx) { ctx->bvh.pairs = ctx->leaf_pairs && ctx->leaf_pairs_resident ? reinterpret_cast<const uint4*>(ctx->pairs.p) : nullptr; }
// The resident leaf records no longer describe the leaf triangles: k_trace tests leaves from BvhTri. Before anything writes
// leaf triangles on the device or replaces them (bvh.h: LeafPair lists the writers). A transforms-only update keeps them: the
// leaf triangles stay, and the wide form collapsed again on the device has the binary tree's leaves, which all have a record.
static void drop_leaf_pairs(sthip_ctx* ctx) {
  ctx->leaf_pairs_resident = false;
  ctx->bvh.pairs = nullptr;
}
static void clear_wide(sthip_ctx* ctx) {  // no 4-wide form: k_trace walks the binary tree (or the 8-wide form)
  ctx->bvh.wide_nodes = nullptr;
  ctx->bvh.wide_entries = nullptr;
  ctx->bvh.wide_root_ref = BVH_INVALID_REF;
  ctx->bvh.wide_stack_depth = 0;
  ctx->wide_node_count = 0;
}
static void clear_wide8(sthip_ctx* ctx) {  // no 8-wide form (ctx->wide8_host stays: a new top level is made behind its bottom levels)
  ctx->bvh.wide8_nodes = nullptr;
  ctx->bvh.wide8_entries = nullptr;
  ctx->bvh.wide8_root = BVH_INVALID_REF;
  ctx->bvh.wide8_stack_depth = 0;
  ctx->wide8_node_count = 0;
}

// The 4-wide form of the tree that is resident now (ctx->nodes / ctx->entries / ctx->bvh.root_ref), made on the device
// (wide.hip): after a GPU build and after a transforms-only update. On failure the binary walk stays (STHIP_OK): a tree whose
// boxes do not fit the wide nodes' grid is still a tree.
static int collapse_resident_tree(sthip_ctx* ctx) {
  clear_wide(ctx);
  const size_t count = (size_t)ctx->bvh_nodes;
  if (count == 0 || ctx->bvh.root_ref == BVH_INVALID_REF || (ctx->bvh.root_ref & BVH_LEAF_BIT) || count * sizeof(WideNode) > 0xFFFFFFFFull) return STHIP_OK;
  if (!ctx->wide_scratch) ctx->wide_scratch = sthip::device_wide_scratch_create();
  HIP_TRY(ctx, ctx->wide_nodes.ensure(count));
  HIP_TRY(ctx, ctx->wide_entries.ensure(std::max<size_t>(1, ctx->top.entries.size())));
  sthip::DeviceWideResult res;
  std::string err;
  if (!sthip::collapse_wide_device(ctx->wide_scratch, reinterpret_cast<const BvhNodeSlot*>(ctx->nodes.p), (uint32_t)count, ctx->entries.p, (uint32_t)ctx->top.entries.size(), ctx->bvh.root_ref,
                                   ctx->bvh.top_is_world_blas != 0, ctx->bvh.stack_depth, ctx->wide_nodes.p, ctx->wide_entries.p, ctx->stream, res, err)) {
    if (getenv("STHIP_VERBOSE")) fprintf(stderr, "[sthip] no wide tree: %s\n", err.c_str());
    return STHIP_OK;
  }
  ctx->bvh.wide_nodes = reinterpret_cast<const uint4*>(ctx->wide_nodes.p);
  ctx->bvh.wide_entries = ctx->wide_entries.p;
  ctx->bvh.wide_root_ref = res.root_ref;
  ctx->bvh.wide_stack_depth = res.stack_depth;
  ctx->wide_node_count = res.node_count;
  ctx->stats.bvh_build_gpu_ms += res.gpu_ms;
  return STHIP_OK;
}

// ---- rigs (sthip_scene_set_rigs / sthip_scene_animate) ----
static void drop_rigs(sthip_ctx* ctx) {
  ctx->rigs.clear();
  ctx->rig_rest.release();
  ctx->rig_targets.release();
  ctx->rig_weights.release();
  ctx->rig_bones.release();
  ctx->rig_bones_host.clear();
  ctx->rig_factors.clear();
}

// The kept scene's vertices are current again: the ranges an animate call wrote on the device come back to the host. Called
// immediately before anything is built from the kept scene.
static int sync_kept_vertices(sthip_ctx* ctx) {
  if (ctx->kept.stale_vertices.empty()) return STHIP_OK;
  if (ctx->kept.valid && ctx->kept.vertices.size() == ctx->vertex_count && ctx->vertices.p) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (k_animate runs on the stream; the copy below does not wait for a non-blocking one)
    for (const auto& r : ctx->kept.stale_vertices)
      if (r.first < r.second && r.second <= ctx->vertex_count)
        HIP_TRY(ctx, hipMemcpy(ctx->kept.vertices.data() + r.first, ctx->vertices.p + r.first, (size_t)(r.second - r.first) * sizeof(sthip_PackedVertexData), hipMemcpyDeviceToHost));
  }
  ctx->kept.stale_vertices.clear();
  return STHIP_OK;
}

// The k_animate launches of an animate call: the bones staged in rig_bones_host go up, then one launch per rig. From the
// first launch on the kept vertices of the rigs' ranges are behind the device's.
static int pose_rigs(sthip_ctx* ctx, const char* call) {
  if (!ctx->rig_bones_host.empty())
    HIP_TRY(ctx, hipMemcpyAsync(ctx->rig_bones.p, ctx->rig_bones_host.data(), ctx->rig_bones_host.size() * sizeof(sthip_TransformData), hipMemcpyHostToDevice, ctx->stream));
  if (ctx->kept.valid)
    for (const auto& r : ctx->rigs) {
      if (!r.count) continue;
      ctx->kept.vertices_written(r.first, r.count);  // (what is left of the range from earlier calls: one entry per range, however often it is posed)
      ctx->kept.stale_vertices.emplace_back(r.first, r.first + r.count);
    }
  HIP_TRY(ctx, hipEventRecord(ctx->edit_ev[0], ctx->stream));
  for (size_t k = 0; k < ctx->rigs.size(); k++) {
    const sthip_ctx::ResidentRig& r = ctx->rigs[k];
    sthip::AnimateRig a;
    a.vertices = ctx->vertices.p + r.first;
    a.rest = ctx->rig_rest.p + r.at;
    for (uint32_t t = 0; t < r.target_count; t++) {
      a.targets[t] = ctx->rig_targets.p + r.targets_at + (size_t)t * r.count;
      a.factors[t] = ctx->rig_factors[k][t];
    }
    a.weights = r.bone_count ? ctx->rig_weights.p + r.at : nullptr;
    a.bones = r.bone_count ? ctx->rig_bones.p + r.bones_at : nullptr;
    a.vertex_count = r.count;
    a.target_count = r.target_count;
    a.bone_count = r.bone_count;
    std::string err;
    if (!sthip::animate_launch(a, ctx->cu_count, ctx->stream, err)) return fail(ctx, STHIP_ERR_HIP, std::string(call) + ": " + err);
  }
  HIP_TRY(ctx, hipEventRecord(ctx->edit_ev[1], ctx->stream));
  return STHIP_OK;
}

// The kept scene's images and tables are current again: texels that came from a device pointer (sthip_scene_set_environment,
// sthip_scene_set_images) and tables that were built on the device come back to the host. Called immediately before anything is
// built from the kept scene.
static int sync_kept_environment(sthip_ctx* ctx) {
  if (ctx->kept.stale_images.empty() && ctx->kept.stale_images1.empty() && !ctx->kept.stale_env_tables) return STHIP_OK;
  if (ctx->kept.valid && ctx->has_scene) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (const uint32_t i : ctx->kept.stale_images) {  // level 0, in the format the image is resident and kept in
      if (i >= ctx->images_host.size() || i >= ctx->kept.image_pixels.size()) continue;
      const DeviceImage& im = ctx->images_host[i];
      const size_t texels = (size_t)im.w[0] * im.h[0];
      if (im.format == STHIP_IMAGE_FORMAT_RGBA8_UNORM) {
        if (ctx->kept.image_bytes[i].size() == texels * 4) HIP_TRY(ctx, hipMemcpy(ctx->kept.image_bytes[i].data(), ctx->image_texels8.p + im.offset[0], texels * 4, hipMemcpyDeviceToHost));
      } else if (ctx->kept.image_pixels[i].size() == texels * 4) {
        HIP_TRY(ctx, hipMemcpy(ctx->kept.image_pixels[i].data(), ctx->image_texels.p + im.offset[0], texels * 16, hipMemcpyDeviceToHost));
      }
    }
    for (const uint32_t i : ctx->kept.stale_images1) {
      if (i >= ctx->images1_host.size() || i >= ctx->kept.image1_pixels.size()) continue;
      const DeviceImage1& im = ctx->images1_host[i];
      const size_t texels = (size_t)im.w * im.h;
      if (im.format == STHIP_IMAGE_FORMAT_R8_UNORM) {
        if (ctx->kept.image1_bytes[i].size() == texels) HIP_TRY(ctx, hipMemcpy(ctx->kept.image1_bytes[i].data(), ctx->image1_texels8.p + im.offset, texels, hipMemcpyDeviceToHost));
      } else if (ctx->kept.image1_pixels[i].size() == texels) {
        HIP_TRY(ctx, hipMemcpy(ctx->kept.image1_pixels[i].data(), ctx->image1_texels.p + im.offset, texels * 4, hipMemcpyDeviceToHost));
      }
    }
    if (ctx->kept.stale_env_tables && ctx->kept.distributions.size() == ctx->distribution_count && ctx->distribution_count)
      HIP_TRY(ctx, hipMemcpy(ctx->kept.distributions.data(), ctx->distributions.p, (size_t)ctx->distribution_count * sizeof(float), hipMemcpyDeviceToHost));
  }
  ctx->kept.stale_images.clear();
  ctx->kept.stale_images1.clear();
  ctx->kept.stale_env_tables = false;
  return STHIP_OK;
}

// What the kept copy is built again from: the kept arrays with the formats their images were uploaded in. The one place that
// brings the kept scene up to date with the device first: vertices, transforms, environment.
static int scene_upload(sthip_ctx* ctx, const sthip_scene_desc* s, const uint8_t* image_formats, const uint8_t* image1_formats);
static int upload_kept_scene(sthip_ctx* ctx) {
  {  // (ranges an animate call posed on the device: the rebuild must see them)
    const int rc = sync_kept_vertices(ctx);
    if (rc != STHIP_OK) return rc;
  }
  {  // (matrices a device-pointer call of sthip_scene_set_transforms left newer than the kept copy)
    const int rc = sync_kept_transforms(ctx);
    if (rc != STHIP_OK) return rc;
  }
  {  // (an environment a device pointer or the device's table build left newer than the kept copy: the rebuild must see it)
    const int rc = sync_kept_environment(ctx);
    if (rc != STHIP_OK) return rc;
  }
  {  // (grids sthip_scene_set_volume built on the device or took from a device pointer)
    const int rc = sync_kept_volumes(ctx);
    if (rc != STHIP_OK) return rc;
  }
  const sthip_scene_desc d = ctx->kept.desc();
  return scene_upload(ctx, &d, ctx->kept.image_formats.empty() ? nullptr : ctx->kept.image_formats.data(), ctx->kept.image1_formats.empty() ? nullptr : ctx->kept.image1_formats.data());
}

int sthip_scene_upload(sthip_ctx* ctx, const sthip_scene_desc* s) { return scene_upload(ctx, s, nullptr, nullptr); }
int sthip_scene_upload_formats(sthip_ctx* ctx, const sthip_scene_desc* s, const uint8_t* image_formats, const uint8_t* image1_formats) { return scene_upload(ctx, s, image_formats, image1_formats); }

// ---- the phases of an upload, in the order scene_upload runs them ----
// What scene_prepare.cpp makes of a checked scene on the host, before anything of the context changes
struct PreparedScene {
  sthip::MaterialAnalysis materials;
  sthip::ImageLayout images;
  sthip::MaskLayout masks;
  std::vector<uint32_t> volume_first_words;
  size_t volume_words = 0;
};
static int prepare_scene(sthip_ctx* ctx, const sthip_scene_desc* s, const uint8_t* image_formats, const uint8_t* image1_formats, PreparedScene& prep) {
  prep.materials = sthip::analyse_materials(*s, image_formats);
  prep.images = sthip::layout_images(*s, image_formats);
  if (prep.images.error) return fail(ctx, STHIP_ERR_UNSUPPORTED, prep.images.error);
  prep.masks = sthip::layout_alpha_masks(*s, image1_formats);
  if (prep.masks.error) return fail(ctx, STHIP_ERR_UNSUPPORTED, prep.masks.error);
  prep.volume_words = sthip::volume_first_words(*s, prep.volume_first_words);
  return STHIP_OK;
}

// The previous scene goes away: from here on no scene is resident until the call has succeeded
static int retire_scene(sthip_ctx* ctx, const sthip_scene_desc* s) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // frames of the previous scene may still be in flight on the caller's stream (device output pointers: sthip_render only
  // enqueues), and the copies of the upload go through the null stream, which a non-blocking stream does not wait for
  // ... and the copy stream of sthip_render_async still reads the staging sets of its frames
  if (const int rc = quiesce(ctx); rc != STHIP_OK) return rc;
  ctx->has_scene = false;
  ctx->scene_serial++;  // (first_hits.h: from here on the resident triangles are not the ones kept hits were traced against)
  sthip::device_refit_invalidate(ctx->refit);  // (the schedule of a refit belongs to the tree that goes away now)
  sthip::device_vertex_adjacency_invalidate(ctx->adjacency);  // (... and the corners of sthip_scene_set_vertices to its index buffer)
  ctx->refit_roots_valid = false;
  // the rigs name vertex ranges of the scene that goes away; a rebuild from the kept copy is the same scene and keeps them
  if (!(ctx->kept.valid && s->gVertices && s->gVertices == ctx->kept.vertices.data())) {
    drop_rigs(ctx);
    ctx->kept.stale_vertices.clear();
  }
  return STHIP_OK;
}

static int upload_vertices_and_indices(sthip_ctx* ctx, const sthip_scene_desc* s) {
  HIP_TRY(ctx, ctx->vertices.ensure(std::max(1u, s->vertex_count)));
  HIP_TRY(ctx, ctx->indices.ensure((size_t)s->indices_bytes + 8));
  if (s->vertex_count) HIP_TRY(ctx, hipMemcpy(ctx->vertices.p, s->gVertices, (size_t)s->vertex_count * sizeof(sthip_PackedVertexData), hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMemset(ctx->indices.p + s->indices_bytes, 0, 8));
  if (s->indices_bytes) HIP_TRY(ctx, hipMemcpy(ctx->indices.p, s->gIndices, s->indices_bytes, hipMemcpyHostToDevice));
  ctx->vertex_count = s->vertex_count;
  ctx->indices_bytes = s->indices_bytes;
  return STHIP_OK;
}

static int build_tree(sthip_ctx* ctx, const sthip_scene_desc* s, sthip::BuiltBvh& built) {
  std::string err;
  // The GPU builder works on the device-resident scene: vertices and indices go up BEFORE the build, and the bottom levels
  // are written in place (lbvh.hip: lbvh_build_device).
  const bool device_build = ctx->bvh_builder == sthip::BVH_BUILDER_LBVH_GPU;
  sthip::DeviceBuildTarget target;
  if (device_build) {
    const int rc = upload_vertices_and_indices(ctx, s);
    if (rc != STHIP_OK) return rc;
    target.vertices = ctx->vertices.p;
    target.vertex_count = s->vertex_count;
    target.indices = ctx->indices.p;
    target.stream = ctx->stream;
    target.algorithm = ctx->lbvh_algorithm;
    target.ploc_radius = ctx->ploc_radius;
    target.sah_top_size = ctx->lbvh_algorithm == 1 ? ctx->sah_top_size : 0;
    target.user = ctx;
    target.reserve = [](void* user, size_t node_capacity, size_t tri_capacity, sthip::DeviceBuildTarget& self) {
      sthip_ctx* c = (sthip_ctx*)user;
      if (c->nodes.ensure(node_capacity) != hipSuccess || c->raw_nodes.ensure(node_capacity) != hipSuccess || c->tris.ensure(tri_capacity) != hipSuccess) return false;
      self.nodes = c->nodes.p;
      self.raw_nodes = c->raw_nodes.p;
      self.tris = c->tris.p;
      return true;
    };
  }
  const auto t_build0 = std::chrono::steady_clock::now();
  if (!sthip::build_scene_bvh(*s, built, err, ctx->bvh_builder, device_build ? &target : nullptr, ctx->embed_leaves && STHIP_NODE_STRIDE == 48))
    return fail(ctx, err.find("only triangle") != std::string::npos ? STHIP_ERR_UNSUPPORTED : STHIP_ERR_INVALID_ARGUMENT, "scene: " + err);

  if (((size_t)built.dev_nodes + built.nodes.size() + 2 * built.entries.size() + 2) * sizeof(BvhNodeSlot) > 0xFFFFFFFFull || ((size_t)built.dev_tris + built.tris.size()) * sizeof(BvhTri) > 0xFFFFFFFFull)
    return fail(ctx, STHIP_ERR_UNSUPPORTED, "scene: the acceleration structure exceeds 4 GiB (the traversal addresses nodes and triangles with 32-bit byte offsets)");
  if (built.stack_depth > STHIP_MAX_STACK_DEPTH) return fail(ctx, STHIP_ERR_UNSUPPORTED, "scene: the acceleration structure is too deep for the traversal stack (use the SAH builder)");
  ctx->stats.bvh_build_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_build0).count();
  ctx->stats.bvh_build_gpu_ms = built.gpu_build_ms;
  return STHIP_OK;
}

static int upload_motion_or_identity(sthip_ctx* ctx, const sthip_TransformData* motion, uint32_t n) {
  if (motion) {
    HIP_TRY(ctx, hipMemcpy(ctx->motion_xf.p, motion, (size_t)n * 48, hipMemcpyHostToDevice));
  } else {
    std::vector<sthip_TransformData> I(n);
    memset(I.data(), 0, (size_t)n * 48);
    for (auto& t : I) t.m[0][0] = t.m[1][1] = t.m[2][2] = 1;
    HIP_TRY(ctx, hipMemcpy(ctx->motion_xf.p, I.data(), (size_t)n * 48, hipMemcpyHostToDevice));
  }
  return STHIP_OK;
}

// gImages: the table and the float texels as scene_prepare.cpp laid them out; an RGBA8 image's level 0 goes up as it is, each
// further level is one launch over the level before it, in stream order (mips.hip)
static int install_images(sthip_ctx* ctx, const sthip_scene_desc* s, sthip::ImageLayout& images) {
  const std::vector<DeviceImage>& table = images.table;
  ctx->image_dims.clear();
  for (uint32_t i = 0; i < s->image_count; i++) ctx->image_dims.emplace_back(s->gImages[i].width, s->gImages[i].height);
  HIP_TRY(ctx, ctx->images.ensure(std::max<size_t>(1, table.size())));
  HIP_TRY(ctx, ctx->image_texels.ensure(std::max<size_t>(1, images.texels.size() / 4)));
  if (!table.empty()) HIP_TRY(ctx, hipMemcpy(ctx->images.p, table.data(), table.size() * sizeof(DeviceImage), hipMemcpyHostToDevice));
  if (!images.texels.empty()) HIP_TRY(ctx, hipMemcpy(ctx->image_texels.p, images.texels.data(), images.texels.size() * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(ctx, ctx->image_texels8.ensure(std::max<size_t>(1, images.texels8)));
  std::string err;
  for (uint32_t i = 0; i < s->image_count; i++) {
    const DeviceImage& im = table[i];
    if (im.format != STHIP_IMAGE_FORMAT_RGBA8_UNORM) continue;
    HIP_TRY(ctx, hipMemcpy(ctx->image_texels8.p + im.offset[0], s->gImages[i].pixels, (size_t)im.w[0] * im.h[0] * 4, hipMemcpyHostToDevice));
    for (uint32_t level = 0; level + 1 < im.levels; level++)
      if (!sthip::mip_rgba8_launch(ctx->image_texels8.p + im.offset[level], im.w[level], im.h[level], ctx->image_texels8.p + im.offset[level + 1], ctx->cu_count, ctx->stream, err)) return fail(ctx, STHIP_ERR_HIP, "scene: " + err);
  }
  if (images.texels8) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->image_count = s->image_count;
  ctx->images_host = std::move(images.table);
  return STHIP_OK;
}

// alpha masks: one-channel images and the per-instance mask index the traversal looks up (the per-triangle uvs it
// interpolates are filled with the shading records, once the triangles are resident)
static int install_alpha_masks(sthip_ctx* ctx, const sthip::MaskLayout& masks, bool any_alpha, const sthip::BuiltBvh& built) {
  HIP_TRY(ctx, ctx->images1.ensure(std::max<size_t>(1, masks.table.size())));
  HIP_TRY(ctx, ctx->image1_texels.ensure(std::max<size_t>(1, masks.texels.size())));
  HIP_TRY(ctx, ctx->tri_uvs.ensure(1));
  if (!masks.table.empty()) HIP_TRY(ctx, hipMemcpy(ctx->images1.p, masks.table.data(), masks.table.size() * sizeof(DeviceImage1), hipMemcpyHostToDevice));
  if (!masks.texels.empty()) HIP_TRY(ctx, hipMemcpy(ctx->image1_texels.p, masks.texels.data(), masks.texels.size() * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(ctx, ctx->image1_texels8.ensure(std::max<size_t>(1, masks.texels8.size())));
  if (!masks.texels8.empty()) HIP_TRY(ctx, hipMemcpy(ctx->image1_texels8.p, masks.texels8.data(), masks.texels8.size(), hipMemcpyHostToDevice));
  HIP_TRY(ctx, ctx->inst_alpha.ensure(std::max<size_t>(1, built.inst_alpha.size())));
  if (!built.inst_alpha.empty()) HIP_TRY(ctx, hipMemcpy(ctx->inst_alpha.p, built.inst_alpha.data(), built.inst_alpha.size() * 4, hipMemcpyHostToDevice));
  ctx->images1_host = masks.table;
  ctx->bvh.inst_alpha = ctx->inst_alpha.p;
  ctx->has_alpha = any_alpha && built.any_alpha;
  ctx->bvh.tri_uv = reinterpret_cast<const float2*>(ctx->tri_uvs.p);
  ctx->bvh.images1 = ctx->images1.p;
  ctx->bvh.image1_texels = ctx->image1_texels.p;
  ctx->bvh.image1_texels8 = ctx->image1_texels8.p;
  ctx->bvh.alpha_test = 0;
  ctx->bvh.flip_uvs = 0;
  return STHIP_OK;
}

// gVolumes: the grids back to back as 32-bit words, and their parsed headers
static int install_volumes(sthip_ctx* ctx, const sthip_scene_desc* s, const std::vector<uint32_t>& first_words, size_t words, sthip::BuiltBvh& built) {
  for (uint32_t i = 0; i < s->volume_count; i++) {
    built.volumes[i].first_word = first_words[i];
    if (i < built.top.volumes.size()) built.top.volumes[i].first_word = first_words[i];  // (the host's copy: read_volume, set_volume)
  }
  HIP_TRY(ctx, ctx->volume_words.ensure(std::max<size_t>(1, words)));
  HIP_TRY(ctx, ctx->volumes.ensure(std::max<size_t>(1, built.volumes.size())));
  for (uint32_t i = 0; i < s->volume_count; i++)
    HIP_TRY(ctx, hipMemcpy(ctx->volume_words.p + built.volumes[i].first_word, s->gVolumes[i].data, (size_t)s->gVolumes[i].bytes, hipMemcpyHostToDevice));
  if (!built.volumes.empty()) HIP_TRY(ctx, hipMemcpy(ctx->volumes.p, built.volumes.data(), built.volumes.size() * sizeof(DeviceVolume), hipMemcpyHostToDevice));
  ctx->volume_count = s->volume_count;
  ctx->bvh.volumes = ctx->volumes.p;
  return STHIP_OK;
}

// The scene's arrays and what the host derived from them, into HBM and into the context
static int install_scene_arrays(sthip_ctx* ctx, const sthip_scene_desc* s, PreparedScene& prep, sthip::BuiltBvh& built) {
  const uint32_t n = s->instance_count;
  sthip::MaterialAnalysis& m = prep.materials;
  HIP_TRY(ctx, ctx->inst_flags.ensure(m.inst_flags.size()));
  HIP_TRY(ctx, hipMemcpy(ctx->inst_flags.p, m.inst_flags.data(), m.inst_flags.size(), hipMemcpyHostToDevice));
  // after build_scene_bvh has succeeded: emitter_bounds reads gIndices at offsets only the builder has validated
  std::vector<EmitterBounds> bounds;
  sthip::emitter_bounds(*s, m.inst_flags, bounds);
  ctx->emitter_count = (uint32_t)bounds.size();
  if (ctx->emitter_count) {
    HIP_TRY(ctx, ctx->emitters.ensure(bounds.size()));
    HIP_TRY(ctx, hipMemcpy(ctx->emitters.p, bounds.data(), bounds.size() * sizeof(EmitterBounds), hipMemcpyHostToDevice));
  }
  ctx->emitters_host = std::move(bounds);
  ctx->inst_flags_host = std::move(m.inst_flags);
  ctx->has_specular = m.has_specular;
  ctx->textured = m.textured;
  ctx->has_spheres = m.has_spheres;
  ctx->has_volumes = m.has_volumes;
  ctx->volume_instances = m.volume_instances;
  ctx->instance_is_volume = std::move(m.instance_is_volume);
  ctx->image_in_material = std::move(m.image_in_material);
  ctx->image_ranges = std::move(m.image_ranges);
  ctx->material_instances.resize(n);
  for (uint32_t i = 0; i < n; i++) ctx->material_instances[i] = sthip::MaterialInstance{s->gInstances[i].packed[0] >> 4, sthip::instance_type(s->gInstances[i])};
  if (ctx->bvh_builder != sthip::BVH_BUILDER_LBVH_GPU) {  // (the GPU builder has them already)
    const int rc = upload_vertices_and_indices(ctx, s);
    if (rc != STHIP_OK) return rc;
  }
  HIP_TRY(ctx, ctx->instances.ensure(n));
  HIP_TRY(ctx, ctx->xf.ensure(n));
  HIP_TRY(ctx, ctx->inv_xf.ensure(n));
  HIP_TRY(ctx, ctx->motion_xf.ensure(n));
  HIP_TRY(ctx, ctx->materials.ensure(s->material_bytes));
  HIP_TRY(ctx, ctx->lights.ensure(std::max(1u, s->light_count)));
  HIP_TRY(ctx, hipMemcpy(ctx->instances.p, s->gInstances, (size_t)n * 16, hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMemcpy(ctx->xf.p, s->gInstanceTransforms, (size_t)n * 48, hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMemcpy(ctx->inv_xf.p, s->gInstanceInverseTransforms, (size_t)n * 48, hipMemcpyHostToDevice));
  int rc = upload_motion_or_identity(ctx, s->gInstanceMotionTransforms, n);
  if (rc != STHIP_OK) return rc;
  HIP_TRY(ctx, hipMemcpy(ctx->materials.p, s->gMaterialData, s->material_bytes, hipMemcpyHostToDevice));
  if (s->light_count) HIP_TRY(ctx, hipMemcpy(ctx->lights.p, s->gLightInstances, (size_t)s->light_count * 4, hipMemcpyHostToDevice));
  ctx->instance_count = n;
  ctx->light_count = s->light_count;
  ctx->materials_host.assign((const uint8_t*)s->gMaterialData, (const uint8_t*)s->gMaterialData + s->material_bytes);
  HIP_TRY(ctx, ctx->distributions.ensure(std::max<size_t>(1, s->distribution_count)));
  if (s->distribution_count) HIP_TRY(ctx, hipMemcpy(ctx->distributions.p, s->gDistributions, (size_t)s->distribution_count * 4, hipMemcpyHostToDevice));
  ctx->distribution_count = s->distribution_count;
  if ((rc = install_images(ctx, s, prep.images)) != STHIP_OK) return rc;
  if ((rc = install_alpha_masks(ctx, prep.masks, m.any_alpha, built)) != STHIP_OK) return rc;
  return install_volumes(ctx, s, prep.volume_first_words, prep.volume_words, built);
}

// The 8-wide form becomes the one k_trace walks: nodes [first, ...) of ctx->wide8_host (the ones before are resident) and
// the entry table go up; the device arrays are large enough
static int install_wide8(sthip_ctx* ctx, size_t first, const std::vector<TlasEntry>& entries, uint32_t root, uint32_t stack_depth) {
  if (ctx->wide8_host.size() > first)
    HIP_TRY(ctx, hipMemcpy(ctx->wide8_nodes.p + first, ctx->wide8_host.data() + first, (ctx->wide8_host.size() - first) * sizeof(Wide8Node), hipMemcpyHostToDevice));
  if (!entries.empty()) HIP_TRY(ctx, hipMemcpy(ctx->wide8_entries.p, entries.data(), entries.size() * sizeof(TlasEntry), hipMemcpyHostToDevice));
  ctx->bvh.wide8_nodes = reinterpret_cast<const uint4*>(ctx->wide8_nodes.p);
  ctx->bvh.wide8_entries = ctx->wide8_entries.p;
  ctx->bvh.wide8_root = root;
  ctx->bvh.wide8_stack_depth = stack_depth;
  ctx->wide8_node_count = ctx->wide8_host.size();
  return STHIP_OK;
}

// The tree: nodes (or embedded units), triangles and entries, the wide form k_trace walks, and ctx->bvh
static int install_tree(sthip_ctx* ctx, sthip::BuiltBvh& built) {
  // the 8-wide form permutes the leaf triangles (bvh_build.h): made before anything of the tree is uploaded
  if (ctx->use_wide == 3 && !ctx->use_treetop && !built.embedded && built.dev_nodes == 0) sthip::build_wide8_bvh(built);
  // headroom: a transforms-only update may build a top level with more inner nodes than this one (at most 2 per entry)
  const size_t nodes_total = (size_t)built.dev_nodes + built.nodes.size(), tris_total = (size_t)built.dev_tris + built.tris.size();
  const size_t nodes_needed = std::max<size_t>(1, built.top.blas_nodes + 2 * built.entries.size() + 2);
  if (built.dev_nodes) {  // the device region is already in place: growing the arrays now would lose it
    if (ctx->nodes.n < std::max(nodes_needed, nodes_total) || ctx->tris.n < std::max<size_t>(1, tris_total)) return fail(ctx, STHIP_ERR_HIP, "scene: the reserved device arrays are too small");
  } else {
    HIP_TRY(ctx, ctx->nodes.ensure(std::max(nodes_needed, nodes_total)));
    HIP_TRY(ctx, ctx->tris.ensure(built.embedded ? 1 : std::max<size_t>(1, tris_total)));
  }
  HIP_TRY(ctx, ctx->entries.ensure(std::max<size_t>(1, built.entries.size())));
  if (built.embedded) {  // one array: packed nodes, and the leaf triangles in the units behind their parents
    std::vector<BvhNodePacked> packed;
    sthip::pack_nodes(built.nodes.data(), built.nodes.size(), packed);
    static_assert(sizeof(BvhNodePacked) == sizeof(BvhTri), "a leaf triangle takes one node unit");
    for (size_t u = 0; u < built.unit_tri.size(); u++)
      if (built.unit_tri[u] != 0xFFFFFFFFu) memcpy(&packed[u], &built.tris[built.unit_tri[u]], sizeof(BvhTri));
    if (!packed.empty()) HIP_TRY(ctx, hipMemcpy(ctx->nodes.p, packed.data(), packed.size() * sizeof(BvhNodePacked), hipMemcpyHostToDevice));
  } else {
    if (!built.nodes.empty()) HIP_TRY(ctx, upload_nodes(ctx, built.dev_nodes, built.nodes.data(), built.nodes.size()));
  }  // (the leaf triangles: below, once build_leaf_pairs has had its say about their order)
  if (!built.entries.empty()) HIP_TRY(ctx, hipMemcpy(ctx->entries.p, built.entries.data(), built.entries.size() * sizeof(TlasEntry), hipMemcpyHostToDevice));
  clear_wide(ctx);
  clear_wide8(ctx);
  drop_leaf_pairs(ctx);  // (they describe the tree that goes away)
  ctx->top_level_static_valid = false;  // (top_level.hip: the per-entry tables belong to the tree that goes away)
  ctx->host_transforms_stale = false;   // (what goes up now is what the host holds)
  ctx->bvh.wide8_tri_min = ctx->tri_min_lanes;
  ctx->wide8_host.clear();
  if (!built.wide8_nodes.empty()) {
    // (room for a rebuilt top level: at most one node per entry and per two entries above them, and a copy of the merged mesh's root)
    HIP_TRY(ctx, ctx->wide8_nodes.ensure(built.top.wide8_blas_nodes + 2 * built.entries.size() + 4));
    HIP_TRY(ctx, ctx->wide8_entries.ensure(std::max<size_t>(1, built.entries.size())));
    ctx->wide8_host = std::move(built.wide8_nodes);
    const int rc = install_wide8(ctx, 0, built.wide8_entries, built.wide8_root, built.wide8_stack_depth);
    if (rc != STHIP_OK) return rc;
  }
  ctx->want_wide = (ctx->use_wide == 1 || (ctx->use_wide == 3 && !ctx->bvh.wide8_nodes) || (ctx->use_wide == 2 && nodes_total * sizeof(BvhNodePacked) > ((size_t)4 << 20))) && !ctx->use_treetop && !built.embedded;
  if (ctx->want_wide && built.dev_nodes == 0) {  // a host-built tree: collapsed on the host from its exact boxes (a device build: below, from the nodes in HBM)
    sthip::build_wide_bvh(built);
    if (!built.wide_nodes.empty() && built.wide_nodes.size() * sizeof(WideNode) <= 0xFFFFFFFFull) {
      sthip::build_leaf_pairs(built);  // (the records are made whatever "leaf_pairs" says: the option picks the kernel, not the tree)
      // (64 bytes per leaf triangle; a device that cannot hold them walks the tree without: the triangles' order stays swapped, which no result depends on)
      if (!built.leaf_pairs.empty() && ctx->pairs.ensure(built.leaf_pairs.size()) != hipSuccess) {
        (void)hipGetLastError();
        built.leaf_pairs.clear();
      }
      if (!built.leaf_pairs.empty()) {
        HIP_TRY(ctx, hipMemcpy(ctx->pairs.p, built.leaf_pairs.data(), built.leaf_pairs.size() * sizeof(LeafPair), hipMemcpyHostToDevice));
        ctx->leaf_pairs_resident = true;
        bind_leaf_pairs(ctx);
        if (getenv("STHIP_VERBOSE"))
          fprintf(stderr, "[sthip] leaf records: %zu single, %zu fan, %zu strip (%zu swapped), %zu two-triangle leaves fit no pattern\n", built.pair_single, built.pair_fan, built.pair_strip, built.pair_swapped,
                  built.pair_unfit);
      }
      HIP_TRY(ctx, ctx->wide_nodes.ensure(built.wide_nodes.size()));
      HIP_TRY(ctx, ctx->wide_entries.ensure(std::max<size_t>(1, built.wide_entries.size())));
      HIP_TRY(ctx, hipMemcpy(ctx->wide_nodes.p, built.wide_nodes.data(), built.wide_nodes.size() * sizeof(WideNode), hipMemcpyHostToDevice));
      if (!built.wide_entries.empty()) HIP_TRY(ctx, hipMemcpy(ctx->wide_entries.p, built.wide_entries.data(), built.wide_entries.size() * sizeof(TlasEntry), hipMemcpyHostToDevice));
      ctx->bvh.wide_nodes = reinterpret_cast<const uint4*>(ctx->wide_nodes.p);
      ctx->bvh.wide_entries = ctx->wide_entries.p;
      ctx->bvh.wide_root_ref = built.wide_root_ref;
      ctx->bvh.wide_stack_depth = built.wide_stack_depth;
      ctx->wide_node_count = built.wide_nodes.size();
    }
  }
  if (!built.embedded && !built.tris.empty()) HIP_TRY(ctx, hipMemcpy(ctx->tris.p + built.dev_tris, built.tris.data(), built.tris.size() * sizeof(BvhTri), hipMemcpyHostToDevice));
  ctx->bvh.nodes = reinterpret_cast<const float4*>(ctx->nodes.p);
  ctx->bvh.tris = built.embedded ? reinterpret_cast<const float4*>(ctx->nodes.p) : reinterpret_cast<const float4*>(ctx->tris.p);
  ctx->bvh.entries = ctx->entries.p;
  ctx->bvh.root_ref = built.root_ref;
  ctx->bvh.top_is_world_blas = built.top_is_world_blas;
  ctx->bvh.stack_depth = built.stack_depth;
  ctx->bvh.scene_cx = built.scene_center[0];
  ctx->bvh.scene_cy = built.scene_center[1];
  ctx->bvh.scene_cz = built.scene_center[2];
  ctx->bvh.scene_radius = built.scene_radius;
  ctx->bvh_nodes = nodes_total;
  ctx->bvh_tris = tris_total;
  ctx->embedded_resident = built.embedded;
  ctx->top = std::move(built.top);
  if (ctx->want_wide && built.dev_nodes != 0) {  // the GPU builder's tree: its wide form is made where the nodes are
    const int rc = collapse_resident_tree(ctx);
    if (rc != STHIP_OK) return rc;
  }
  // the host's copy of the unpacked nodes, with room for a rebuilt top level
  // (only the treetop selection reads it: without the treetop a device-resident build copies no node to the host at all)
  ctx->nodes_host.n = 0;
  if (ctx->use_treetop) {
    HIP_TRY(ctx, ctx->nodes_host.ensure(std::max<size_t>(nodes_total, ctx->nodes.n)));
    if (built.dev_nodes) HIP_TRY(ctx, hipMemcpy(ctx->nodes_host.p, ctx->raw_nodes.p, (size_t)built.dev_nodes * sizeof(BvhNode), hipMemcpyDeviceToHost));
    if (!built.nodes.empty()) memcpy(ctx->nodes_host.p + built.dev_nodes, built.nodes.data(), built.nodes.size() * sizeof(BvhNode));
    ctx->nodes_host.n = nodes_total;
  }
  return STHIP_OK;
}

// k_fill_tri_shade over the first `units` resident leaf triangles (`is_tri`: which units are triangles, NULL = all)
static int launch_fill_tri_shade(sthip_ctx* ctx, size_t units, const uint8_t* is_tri) {
  hipLaunchKernelGGL(k_fill_tri_shade, dim3(grid_for(ctx, units)), dim3(STHIP_BLOCK), 0, ctx->stream, reinterpret_cast<const BvhTri*>(ctx->bvh.tris), (uint32_t)units, is_tri, ctx->vertices.p, ctx->vertex_count,
                     ctx->indices.p, ctx->indices_bytes, ctx->tri_shade.p, ctx->has_alpha ? ctx->tri_uvs.p : nullptr);
  HIP_TRY(ctx, hipGetLastError());
  return STHIP_OK;
}

// the shading records beside the leaf triangles (bvh.h: BvhTriShade), from the triangles as they lie in HBM now
static int derive_leaf_records(sthip_ctx* ctx, const sthip::BuiltBvh& built) {
  const size_t units = built.embedded ? ctx->bvh_nodes : ctx->bvh_tris;  // (embedded leaves: a triangle is a unit of the node array; the units that are nodes get a record nobody reads)
  HIP_TRY(ctx, ctx->tri_shade.ensure(std::max<size_t>(1, units)));
  if (ctx->has_alpha) {  // the uvs the traversal's alpha test interpolates (gAlphaTest, intersection.hlsli:117-131), in the same order
    HIP_TRY(ctx, ctx->tri_uvs.ensure(std::max<size_t>(1, units)));
    ctx->bvh.tri_uv = reinterpret_cast<const float2*>(ctx->tri_uvs.p);
  }
  if (units && ctx->vertex_count) {
    DevBuf<uint8_t> is_tri;  // embedded leaves: which units are triangles
    if (built.embedded) {
      std::vector<uint8_t> flags(units, 0);
      for (size_t u = 0; u < built.unit_tri.size() && u < units; u++) flags[u] = built.unit_tri[u] != 0xFFFFFFFFu;
      HIP_TRY(ctx, is_tri.ensure(units));
      HIP_TRY(ctx, hipMemcpy(is_tri.p, flags.data(), units, hipMemcpyHostToDevice));
    }
    const int rc = launch_fill_tri_shade(ctx, units, is_tri.p);
    if (rc != STHIP_OK) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (`is_tri` goes out of scope)
  }
  return STHIP_OK;
}

// sthip.h. check -> prepare -> retire the previous scene -> build -> install -> derive -> keep: a call refused by the check or
// the preparation leaves the context as it was; a failure from the build onward leaves no scene resident.
static int scene_upload(sthip_ctx* ctx, const sthip_scene_desc* s, const uint8_t* image_formats, const uint8_t* image1_formats) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  int rc = STHIP_OK;
  std::string why;
  if (!sthip::check_scene(s, image_formats, image1_formats, rc, why)) return fail(ctx, rc, why);
  PreparedScene prep;
  sthip::BuiltBvh built;
  if ((rc = prepare_scene(ctx, s, image_formats, image1_formats, prep)) != STHIP_OK) return rc;
  if ((rc = retire_scene(ctx, s)) != STHIP_OK) return rc;
  if ((rc = build_tree(ctx, s, built)) != STHIP_OK) return rc;
  if ((rc = install_scene_arrays(ctx, s, prep, built)) != STHIP_OK) return rc;
  if ((rc = install_tree(ctx, built)) != STHIP_OK) return rc;
  if ((rc = derive_leaf_records(ctx, built)) != STHIP_OK) return rc;
  if ((rc = configure_stack(ctx)) != STHIP_OK) return rc;
  ctx->has_scene = true;
  ctx->reuse_grids_valid = false;  // (stored samples name materials and lights of the scene they were taken in)
  if (ctx->keep_scene) {
    // (a rebuild from the kept copy itself keeps nothing anew; its stale marks are clear already: upload_kept_scene, the only
    // caller that passes the kept arrays, has run the three syncs, and each clears its marks)
    if (s->gVertices != ctx->kept.vertices.data() || !ctx->kept.valid) ctx->kept.keep(*s, image_formats, image1_formats);
  } else {
    ctx->kept = KeptScene();
  }
  if (getenv("STHIP_VERBOSE"))
    fprintf(stderr, "[sthip] bvh (%s): %zu nodes, %zu tris, %zu top-level entries, stack depth %u (%zu B LDS / block%s, treetop %u nodes), %d trace blocks / CU, build %.1f ms (GPU kernels %.2f ms)\n",
            ctx->bvh_builder ? "lbvh/gpu" : "sah/host", (size_t)ctx->bvh_nodes, (size_t)ctx->bvh_tris, built.entries.size(), built.stack_depth, stack_bytes(ctx), ctx->bvh.spill ? ", bounded" : "", ctx->bvh.top_count,
            trace_occupancy(ctx, trace_lds_bytes(ctx)), ctx->stats.bvh_build_ms, ctx->stats.bvh_build_gpu_ms);
  return STHIP_OK;
}

static unsigned long long* queue_ctl_host(unsigned long long* qctl, uint32_t kind, uint32_t depth) {
  return qctl + (size_t)((kind * 64u + depth) * QUEUE_SEGMENTS) * QCTL_STRIDE;
}
static uint32_t grid_for(const sthip_ctx* ctx, size_t n) {
  const size_t blocks = (n + STHIP_BLOCK - 1) / STHIP_BLOCK;
  const size_t cap = (size_t)ctx->cu_count * 32;  // grid-stride beyond this
  return (uint32_t)std::max<size_t>(1, std::min(blocks, cap));
}
// Persistent trace kernels: as many blocks as are resident at once (LDS stack and VGPRs bound it).
static int trace_occupancy(const sthip_ctx* ctx, size_t lds_bytes) {  // resident k_trace blocks per CU with that much dynamic LDS
  int per_cu = 0;
  hipError_t e;
  e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, trace_kernel(ctx->bvh, false, false, ctx->use_treetop), STHIP_BLOCK, lds_bytes);
  return e == hipSuccess ? per_cu : 0;
}
static uint32_t trace_grid(sthip_ctx* ctx, size_t lds_bytes) {
  int per_cu = trace_occupancy(ctx, lds_bytes);
  if (per_cu < 1) per_cu = 2;
  if (ctx->trace_blocks_per_cu) per_cu = (int)ctx->trace_blocks_per_cu;
  return (uint32_t)(ctx->cu_count * per_cu);
}
static size_t stack_bytes(const sthip_ctx* ctx) { return (size_t)ctx->bvh.lds_levels * STHIP_BLOCK * (ctx->bvh.wide8_nodes ? sizeof(uint2) : sizeof(uint32_t)); }  // (the 8-wide walk's entries are 64-bit groups)

// LDS of one k_trace block: the per-lane stacks and, behind them, the treetop
static size_t trace_lds_bytes(const sthip_ctx* ctx) { return stack_bytes(ctx) + (size_t)ctx->bvh.top_count * sizeof(BvhNodePacked); }

// Decides how the traversal stack of the current tree is held: all of it in LDS, or lds_stack_cap levels there and the
// full height in global memory for the rays that overflow. Then the treetop takes the LDS that is left.
static int configure_stack(sthip_ctx* ctx) {
  // (the wide walk pushes up to three children per level, and every step writes the three levels from `top` on)
  const uint32_t need = ctx->bvh.wide8_nodes ? ctx->bvh.wide8_stack_depth : ctx->bvh.wide_nodes ? ctx->bvh.wide_stack_depth + 3u : ctx->bvh.stack_depth;
  // (a 64-bit entry counts as two levels of the limits, which are about LDS bytes)
  const bool bounded = ctx->bvh.wide8_nodes ? 2u * need > ctx->lds_stack_threshold : need > ctx->lds_stack_threshold;
  ctx->bvh.lds_levels = bounded ? (ctx->bvh.wide8_nodes ? std::max(4u, ctx->lds_stack_cap / 2u) : ctx->lds_stack_cap) : need;
  ctx->bvh.spill = nullptr;
  if (bounded) {
    // one column per lane of the largest grid a trace launch can have (persistent: resident blocks; ray batches use it too)
    HIP_TRY(ctx, ctx->spill.ensure((size_t)ctx->cu_count * 8 * STHIP_BLOCK * ctx->bvh.stack_depth));
    ctx->bvh.spill = ctx->spill.p;
  }
  return refresh_treetop(ctx);
}

// (Re)builds the treetop for the current top level: as many nodes as fit into the LDS the stacks leave free at the
// occupancy the kernel's registers allow anyway (the treetop must not cost a resident block).
static int refresh_treetop(sthip_ctx* ctx) {
  ctx->bvh.top_nodes = nullptr;
  ctx->bvh.top_entries = ctx->bvh.entries;
  ctx->bvh.top_root_ref = ctx->bvh.root_ref;
  ctx->bvh.top_count = 0;
  if (!ctx->use_treetop || ctx->nodes_host.empty()) return STHIP_OK;
  int per_cu = 0;
  const size_t stack = stack_bytes(ctx);
  per_cu = trace_occupancy(ctx, stack);
  if (per_cu < 1) return STHIP_OK;
  if (ctx->trace_blocks_per_cu) per_cu = (int)ctx->trace_blocks_per_cu;
  const size_t lds_per_cu = 160 * 1024, per_block = lds_per_cu / (size_t)per_cu;
  if (per_block < stack + 2048) return STHIP_OK;
  uint32_t capacity = (uint32_t)std::min<size_t>((per_block - stack - 1024) / sizeof(BvhNodePacked), 2048);
  while (capacity >= 16) {  // the allocation granularity is the runtime's: ask it
    int got = 0;
    got = trace_occupancy(ctx, stack + (size_t)capacity * sizeof(BvhNodePacked));
    if (got >= per_cu) break;
    capacity -= 16;
  }
  if (capacity < 16) return STHIP_OK;
  sthip::Treetop tt;
  sthip::build_treetop(ctx->nodes_host.data(), (size_t)ctx->bvh_nodes, ctx->top.entries, ctx->bvh.root_ref, capacity, tt);
  if (tt.nodes.empty()) return STHIP_OK;
  HIP_TRY(ctx, ctx->top_nodes.ensure(tt.nodes.size()));
  HIP_TRY(ctx, ctx->top_entries.ensure(std::max<size_t>(1, tt.entries.size())));
  {
    std::vector<BvhNodePacked> packed;
    sthip::pack_nodes(tt.nodes.data(), tt.nodes.size(), packed);
    HIP_TRY(ctx, hipMemcpy(ctx->top_nodes.p, packed.data(), packed.size() * sizeof(BvhNodePacked), hipMemcpyHostToDevice));
  }
  if (!tt.entries.empty()) HIP_TRY(ctx, hipMemcpy(ctx->top_entries.p, tt.entries.data(), tt.entries.size() * sizeof(TlasEntry), hipMemcpyHostToDevice));
  ctx->bvh.top_nodes = reinterpret_cast<const float4*>(ctx->top_nodes.p);
  ctx->bvh.top_entries = ctx->top_entries.p;
  ctx->bvh.top_root_ref = tt.root_ref;
  ctx->bvh.top_count = (uint32_t)tt.nodes.size();
  return STHIP_OK;
}

int sthip_trace_rays(sthip_ctx* ctx, const sthip_ray* rays, uint32_t ray_count, sthip_hit* hits, uint32_t any_hit, uint32_t device_ptrs) {
  if (!ctx || !rays || !hits) return STHIP_ERR_INVALID_ARGUMENT;
  if (!ctx->has_scene) return fail(ctx, STHIP_ERR_NO_SCENE, "no scene uploaded");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (ray_count == 0) return STHIP_OK;
  const sthip_ray* d_rays = rays;
  sthip_hit* d_hits = hits;
  DevBuf<sthip_ray>& rb = ctx->ray_staging;  // kept in the context: no hipMalloc / hipFree per call
  DevBuf<sthip_hit>& hb = ctx->hit_staging;
  if (!device_ptrs) {
    HIP_TRY(ctx, rb.ensure(ray_count));
    HIP_TRY(ctx, hb.ensure(ray_count));
    HIP_TRY(ctx, hipMemcpyAsync(rb.p, rays, (size_t)ray_count * sizeof(sthip_ray), hipMemcpyHostToDevice, ctx->stream));
    d_rays = rb.p;
    d_hits = hb.p;
  }
  HIP_TRY(ctx, ctx->counters.ensure(CNT_TOTAL));
  HIP_TRY(ctx, hipMemsetAsync(ctx->counters.p, 0, CNT_TOTAL * sizeof(unsigned long long), ctx->stream));
  // bounded stacks: the batch kernel walks with full-height stacks in global memory, one column per lane of a grid the spill buffer covers
  const uint32_t grid = ctx->bvh.spill ? std::min<uint32_t>(grid_for(ctx, ray_count), (uint32_t)ctx->cu_count * 8u) : grid_for(ctx, ray_count);
  const size_t lds = ctx->bvh.spill ? 0 : stack_bytes(ctx);
  DeviceBvh bvh = ctx->bvh;
  bvh.alpha_test = (ctx->has_alpha && (any_hit & 2u)) ? 1u : 0u;
  bvh.flip_uvs = (any_hit & 4u) ? 1u : 0u;
  any_hit &= 1u;
  launch_kernel(STHIP_KERNEL2(k_trace_batch, any_hit != 0, ctx->count_traversal), grid, lds, ctx->stream, bvh, d_rays, ray_count, d_hits, ctx->counters.p);
  HIP_TRY(ctx, hipGetLastError());
  if (!device_ptrs) {
    HIP_TRY(ctx, hipMemcpyAsync(hits, hb.p, (size_t)ray_count * sizeof(sthip_hit), hipMemcpyDeviceToHost, ctx->stream));
    std::vector<unsigned long long> c(CNT_TOTAL);
    HIP_TRY(ctx, hipMemcpyAsync(c.data(), ctx->counters.p, CNT_TOTAL * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stats.nodes_visited = c[CNT_NODES];
    ctx->stats.tris_tested = c[CNT_TRIS];
    ctx->stats.nodes_visited_shadow = c[CNT_NODES + 1];
    ctx->stats.tris_tested_shadow = c[CNT_TRIS + 1];
  }
  return STHIP_OK;
}

// A new top level over bottom levels that stay where they are (a transforms-only update; a refit, whose bottom levels have new
// boxes): entries and top-level nodes into HBM, the scene bounds, and the forms derived from the binary tree made again.
static int finish_top_level(sthip_ctx* ctx, const BvhNode* tlas_nodes, size_t tlas_count, uint32_t root_ref, uint32_t top_is_world, uint32_t stack_depth, const float center[3], float radius);
static int install_top_level(sthip_ctx* ctx, sthip::TopLevelState& next, const std::vector<BvhNode>& tlas, uint32_t root_ref, uint32_t top_is_world, uint32_t stack_depth, const float center[3],
                             float radius) {
  if (!next.entries.empty()) HIP_TRY(ctx, hipMemcpy(ctx->entries.p, next.entries.data(), next.entries.size() * sizeof(TlasEntry), hipMemcpyHostToDevice));
  if (!tlas.empty()) HIP_TRY(ctx, upload_nodes(ctx, next.blas_nodes, tlas.data(), tlas.size()));
  ctx->top = std::move(next);
  return finish_top_level(ctx, tlas.data(), tlas.size(), root_ref, top_is_world, stack_depth, center, radius);
}
// ... once the entries and the packed top-level nodes are resident and ctx->top describes them (the device builder of
// sthip_scene_set_transforms comes here directly; `tlas_nodes` may then be NULL unless a host-made layout needs them)
static int finish_top_level(sthip_ctx* ctx, const BvhNode* tlas_nodes, size_t tlas_count, uint32_t root_ref, uint32_t top_is_world, uint32_t stack_depth, const float center[3], float radius) {
  const uint32_t blas_nodes = ctx->top.blas_nodes;
  ctx->bvh.root_ref = root_ref;
  ctx->bvh.top_is_world_blas = top_is_world;
  ctx->bvh.stack_depth = stack_depth;
  ctx->bvh.scene_cx = center[0];
  ctx->bvh.scene_cy = center[1];
  ctx->bvh.scene_cz = center[2];
  ctx->bvh.scene_radius = radius;
  ctx->bvh_nodes = blas_nodes + tlas_count;
  if (ctx->nodes_host.n && ctx->nodes_host.cap >= (size_t)blas_nodes + tlas_count) {
    if (tlas_count) memcpy(ctx->nodes_host.p + blas_nodes, tlas_nodes, tlas_count * sizeof(BvhNode));
    ctx->nodes_host.n = std::max(ctx->nodes_host.n, (size_t)blas_nodes + tlas_count);
  }
  // the wide form was made from the old top level: made again from the nodes in HBM (the bottom levels come out as before,
  // the top level new), so a moved scene keeps the walk it was uploaded with
  clear_wide(ctx);
  if (ctx->bvh.wide8_nodes) {  // the 8-wide form: its top level again, on the host (a node per few entries), behind the bottom levels' nodes
    std::vector<TlasEntry> entries8;
    uint32_t root8 = BVH_INVALID_REF, depth8 = 0;
    clear_wide8(ctx);
    if (sthip::build_wide8_top(ctx->top, tlas_nodes, ctx->top.blas_nodes, root_ref, top_is_world != 0, ctx->wide8_host, entries8, root8, depth8) && ctx->wide8_host.size() <= ctx->wide8_nodes.n &&
        entries8.size() <= ctx->wide8_entries.n) {
      const int rc = install_wide8(ctx, ctx->top.wide8_blas_nodes, entries8, root8, depth8);
      if (rc != STHIP_OK) return rc;
    } else {  // (a top level that cannot take the form: the 4-wide one from here on)
      ctx->want_wide = !ctx->use_treetop;
    }
  }
  if (ctx->want_wide && !ctx->bvh.wide8_nodes) {
    const int rc = collapse_resident_tree(ctx);
    if (rc != STHIP_OK) {  // (an allocation of the collapse failed: the new binary tree is resident and walked; its stack must be configured for it)
      const std::string why = ctx->error;
      (void)configure_stack(ctx);
      ctx->error = why;
      return rc;
    }
  }
  return configure_stack(ctx);
}

// The host's copies of the instance matrices are current again: after a device-pointer call of sthip_scene_set_transforms, or
// one that derived an array, the kept scene's three arrays and the inverses in ctx->top.entries come back from the device.
// Called immediately before their next reader, as sync_kept_vertices is.
static int sync_kept_transforms(sthip_ctx* ctx) {
  if (!ctx->host_transforms_stale) return STHIP_OK;
  const uint32_t n = ctx->instance_count;
  if (ctx->has_scene && n && ctx->xf.p && ctx->inv_xf.p && ctx->motion_xf.p) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<sthip_TransformData> xf(n), inv(n), motion(n);
    HIP_TRY(ctx, hipMemcpy(xf.data(), ctx->xf.p, (size_t)n * 48, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(inv.data(), ctx->inv_xf.p, (size_t)n * 48, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(motion.data(), ctx->motion_xf.p, (size_t)n * 48, hipMemcpyDeviceToHost));
    if (ctx->kept.valid && ctx->kept.instances.size() == n) ctx->kept.set_transforms(xf.data(), inv.data(), motion.data(), n);
    for (TlasEntry& e : ctx->top.entries)
      if (e.identity != TLAS_ENTRY_IDENTITY && e.id_bits < n) memcpy(e.inv, &inv[e.id_bits], 48);
  }
  ctx->host_transforms_stale = false;
  return STHIP_OK;
}

// sthip_scene_update_transforms, and the host builder of sthip_scene_set_transforms once its matrices are host arrays
static int update_transforms_host(sthip_ctx* ctx, const std::string& call, const sthip_TransformData* xf, const sthip_TransformData* inv, const sthip_TransformData* motion, uint32_t instance_count,
                                  sthip_transforms_info* info) {
  ctx->scene_serial++;  // (first_hits.h; a refused call costs one trace of the first bounce)
  sthip::TopLevelState next = ctx->top;  // nothing changes unless everything succeeds
  std::vector<BvhNode> tlas;
  uint32_t root_ref = 0, top_is_world = 1, stack_depth = 4;
  float center[3] = {ctx->bvh.scene_cx, ctx->bvh.scene_cy, ctx->bvh.scene_cz}, radius = ctx->bvh.scene_radius;
  std::string err;
  if (!sthip::rebuild_top_level(next, xf, inv, instance_count, tlas, root_ref, top_is_world, stack_depth, center, radius, err)) {
    // An instance of the merged world-space mesh (identity transform at upload) moved: the tree that is resident cannot follow,
    // the scene is built again from the copy kept at upload, with the new transforms — the configured builder ("bvh_builder" = 1:
    // ~10 ms per million triangles on the device), everything else as uploaded. Without the copy ("keep_scene" = 0) it is refused.
    if (ctx->kept.valid && ctx->kept.instances.size() == instance_count) {
      ctx->kept.set_transforms(xf, inv, motion, instance_count);
      ctx->host_transforms_stale = false;  // (all three arrays of the kept scene are the call's now; the upload makes the entries)
      ctx->stats.full_rebuilds++;
      if (info) info->rebuilt = 1;
      return upload_kept_scene(ctx);
    }
    return fail(ctx, STHIP_ERR_UNSUPPORTED, call + err);
  }
  if (stack_depth > STHIP_MAX_STACK_DEPTH) return fail(ctx, STHIP_ERR_UNSUPPORTED, call + "the new top level is too deep for the traversal stack");
  if ((size_t)next.blas_nodes + tlas.size() > ctx->nodes.n) return fail(ctx, STHIP_ERR_UNSUPPORTED, call + "the new top level does not fit: upload the scene again");
  // frames in flight still read the old top level (sthip_render_async: their copies too, so that their tickets are complete)
  if (const int rc = quiesce(ctx); rc != STHIP_OK) return rc;
  const uint32_t n = instance_count;
  HIP_TRY(ctx, hipMemcpy(ctx->xf.p, xf, (size_t)n * 48, hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMemcpy(ctx->inv_xf.p, inv, (size_t)n * 48, hipMemcpyHostToDevice));
  {
    const int rc = upload_motion_or_identity(ctx, motion, n);
    if (rc != STHIP_OK) return rc;
  }
  // the kept scene follows: a later rebuild from it (sthip_scene_update_vertices on a layout it does not refit) must find the
  // instances where they are now, and the refit takes the transforms of its top level from here instead of from the device
  if (ctx->kept.valid && ctx->kept.instances.size() == n) ctx->kept.set_transforms(xf, inv, motion, n);
  ctx->host_transforms_stale = false;  // (the kept arrays and every entry's inverse are the call's)
  if (info) {
    info->top_level_nodes = (uint32_t)tlas.size();
    info->top_level_depth = stack_depth - next.blas_depth - 3;
  }
  return install_top_level(ctx, next, tlas, root_ref, top_is_world, stack_depth, center, radius);
}

int sthip_scene_update_transforms(sthip_ctx* ctx, const sthip_TransformData* xf, const sthip_TransformData* inv, const sthip_TransformData* motion, uint32_t instance_count) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  if (!ctx->has_scene) return fail(ctx, STHIP_ERR_NO_SCENE, "sthip_scene_update_transforms before sthip_scene_upload");
  if (!xf || !inv) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_scene_update_transforms: transforms and inverse transforms are required");
  if (instance_count != ctx->instance_count) return fail(ctx, STHIP_ERR_UNSUPPORTED, "sthip_scene_update_transforms: the instance count changed: upload the scene again");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return update_transforms_host(ctx, "sthip_scene_update_transforms: ", xf, inv, motion, instance_count, nullptr);
}

// ---- the grids of a resident scene: sthip_scene_set_volume / sthip_scene_read_volume ----
// The kept scene's grids are current again: those a set_volume call left newer on the device come back. Called immediately
// before anything is built from the kept scene (upload_kept_scene), as sync_kept_environment is.
static int sync_kept_volumes(sthip_ctx* ctx) {
  if (ctx->kept.stale_volumes.empty()) return STHIP_OK;
  // (no scene, or a kept copy of another one: nothing to fetch from; the marks stay until the next upload keeps a scene,
  // so that nothing is ever built from a grid known to be old)
  if (!ctx->has_scene || !ctx->kept.valid || ctx->kept.volume_bytes.size() != ctx->top.volumes.size()) return STHIP_OK;
  {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (const uint32_t i : ctx->kept.stale_volumes) {
      if (i >= ctx->top.volumes.size()) continue;
      const DeviceVolume& v = ctx->top.volumes[i];
      ctx->kept.volume_bytes[i].resize(v.bytes);
      HIP_TRY(ctx, hipMemcpy(ctx->kept.volume_bytes[i].data(), ctx->volume_words.p + v.first_word, v.bytes, hipMemcpyDeviceToHost));
      ctx->kept.volumes[i] = sthip_volume_desc{ctx->kept.volume_bytes[i].data(), v.bytes};
    }
  }
  ctx->kept.stale_volumes.clear();
  return STHIP_OK;
}

int sthip_scene_read_volume(sthip_ctx* ctx, uint32_t volume_index, void* dst, uint64_t capacity, uint64_t* bytes) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  if (!ctx->has_scene) return fail(ctx, STHIP_ERR_NO_SCENE, "sthip_scene_read_volume before sthip_scene_upload");
  if (volume_index >= ctx->top.volumes.size()) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_scene_read_volume: volume_index is out of range");
  const DeviceVolume& v = ctx->top.volumes[volume_index];
  if (bytes) *bytes = v.bytes;
  if (!dst || capacity < v.bytes) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_scene_read_volume: the grid has " + std::to_string(v.bytes) + " bytes, capacity is " + std::to_string(capacity));
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipMemcpy(dst, ctx->volume_words.p + v.first_word, v.bytes, hipMemcpyDeviceToHost));
  return STHIP_OK;
}

int sthip_scene_set_volume(sthip_ctx* ctx, uint32_t volume_index, const sthip_volume_source* src, sthip_volume_info* info) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  const auto t0 = std::chrono::steady_clock::now();
  const std::string call = "sthip_scene_set_volume: ";
  if (!ctx->has_scene) return fail(ctx, STHIP_ERR_NO_SCENE, "sthip_scene_set_volume before sthip_scene_upload");
  if (!src || src->struct_size != sizeof(sthip_volume_source)) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, call + "struct_size is not sizeof(sthip_volume_source)");
  if (volume_index >= ctx->top.volumes.size()) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, call + "volume_index is out of range");
  if ((src->data != nullptr) == (src->dense != nullptr)) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, call + "exactly one of data and dense must be given");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = make_edit_events(ctx)) != STHIP_OK) return rc;
  // ---- every check, the build and its read-back: nothing resident is touched ----
  sthip_volume_info local{};
  DeviceVolume parsed;
  const void* grid = nullptr;  // where the new grid's bytes lie
  hipMemcpyKind kind = hipMemcpyHostToDevice;
  uint64_t grid_bytes = 0;
  float build_ms = 0;
  DevBuf<float> staged;
  std::string err;
  if (src->dense) {
    sthip::VolumeBuildInput in{};
    sthip::VolumeBuildCounts c{};
    sthip::VolumeHeader header;
    float scan_ms = 0, emit_ms = 0;
    if ((rc = dense_volume_scan(ctx, "sthip_scene_set_volume", src->dense, staged, in, c, header, &local, scan_ms)) != STHIP_OK) return rc;
    void* target = sthip::volume_build_staging(ctx->volume_build, local.bytes, err);
    if (!target) return fail(ctx, STHIP_ERR_HIP, call + err);
    if (!sthip::volume_build_emit(ctx->volume_build, in, c, header, target, ctx->stream, emit_ms, err)) return fail(ctx, STHIP_ERR_HIP, call + err);
    if (!sthip::parse_volume_header((const uint8_t*)header.w, sizeof(header), local.bytes, parsed, err)) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, call + err);
    grid = target, kind = hipMemcpyDeviceToDevice, grid_bytes = local.bytes, build_ms = scan_ms + emit_ms;
  } else {
    const uint64_t n = src->bytes;
    std::vector<uint8_t> head;  // a device pointer: the header, the tree and the root come to the host for the checks
    const uint8_t* b = (const uint8_t*)src->data;
    uint64_t have = n;
    if (src->data_is_device) {
      if ((uintptr_t)src->data & 3u) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, call + "data is a device pointer that is not 4-byte aligned");
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      have = std::min<uint64_t>(n, 672 + 64);
      head.resize(have);
      if (have) HIP_TRY(ctx, hipMemcpy(head.data(), src->data, have, hipMemcpyDeviceToHost));
      uint64_t root = 0;
      if (have >= 672 + 32) memcpy(&root, head.data() + 672 + 24, 8);
      const uint64_t want = root <= n ? std::min<uint64_t>(n, 672 + root + 64) : have;
      if (want > have) {
        head.resize(want);
        HIP_TRY(ctx, hipMemcpy(head.data() + have, (const uint8_t*)src->data + have, want - have, hipMemcpyDeviceToHost));
        have = want;
      }
      b = head.data();
      kind = hipMemcpyDeviceToDevice;
    }
    if (!sthip::parse_volume_header(b, have, n, parsed, err)) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, call + err);
    grid = src->data, grid_bytes = n;
    local.bytes = n;
    for (int a = 0; a < 3; a++) local.bbox_min[a] = parsed.bbox_min[a], local.bbox_max[a] = parsed.bbox_max[a];
    local.max = parsed.root_max;
  }
  // the new layout: the grids back to back, as the upload lays them out
  std::vector<DeviceVolume> next = ctx->top.volumes;
  parsed.first_word = 0;
  next[volume_index] = parsed;
  uint64_t words = 0;
  for (DeviceVolume& v : next) {
    v.first_word = (uint32_t)words;
    words += v.bytes / 4;
  }
  if (words > 0xFFFFFFFFull) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, call + "gVolumes exceed 16 GiB");
  DevBuf<uint32_t> fresh;
  HIP_TRY(ctx, fresh.ensure(std::max<uint64_t>(1, words)));
  // ---- the install: frames in flight still read the old words ----
  if ((rc = quiesce(ctx)) != STHIP_OK) return rc;
  HIP_TRY(ctx, hipEventRecord(ctx->edit_ev[0], ctx->stream));
  auto lost = [&](int code) {  // (a failure from here on: the resident scene is neither the old nor the new one)
    ctx->has_scene = false;
    ctx->kept = KeptScene();  // (its copy of this grid may be the old one: nothing may be built from it any more)
    return code;
  };
  for (size_t i = 0; i < next.size(); i++) {
    const hipError_t e = i == volume_index ? hipMemcpyAsync(fresh.p + next[i].first_word, grid, grid_bytes, kind, ctx->stream)
                                           : hipMemcpyAsync(fresh.p + next[i].first_word, ctx->volume_words.p + ctx->top.volumes[i].first_word, next[i].bytes, hipMemcpyDeviceToDevice, ctx->stream);
    if (e != hipSuccess) return lost(fail(ctx, STHIP_ERR_HIP, call + hipGetErrorString(e)));
  }
  if (hipMemcpyAsync(ctx->volumes.p, next.data(), next.size() * sizeof(DeviceVolume), hipMemcpyHostToDevice, ctx->stream) != hipSuccess || hipEventRecord(ctx->edit_ev[1], ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess)
    return lost(fail(ctx, STHIP_ERR_HIP, call + "installing the grids failed"));
  std::swap(ctx->volume_words.p, fresh.p);  // (the old words are freed with `fresh`)
  std::swap(ctx->volume_words.n, fresh.n);
  ctx->top.volumes = next;
  ctx->reuse_grids_valid = false;  // (stored samples were taken in the old medium)
  if (ctx->kept.valid && ctx->kept.volume_bytes.size() == next.size()) {
    if (!src->dense && !src->data_is_device) {
      ctx->kept.volume_bytes[volume_index].assign((const uint8_t*)src->data, (const uint8_t*)src->data + grid_bytes);
      ctx->kept.volumes[volume_index] = sthip_volume_desc{ctx->kept.volume_bytes[volume_index].data(), grid_bytes};
      ctx->kept.stale_volumes.erase(volume_index);
    } else {
      ctx->kept.stale_volumes.insert(volume_index);
    }
  }
  // the entry boxes of the volume instances, the top level and the scene bounds: the path sthip_scene_update_transforms
  // takes, with the matrices that are resident
  const uint32_t n = ctx->instance_count;
  if (n) {
    std::vector<sthip_TransformData> xf(n), inv(n), motion(n);
    if (hipMemcpy(xf.data(), ctx->xf.p, (size_t)n * 48, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(inv.data(), ctx->inv_xf.p, (size_t)n * 48, hipMemcpyDeviceToHost) != hipSuccess ||
        (ctx->motion_xf.p && hipMemcpy(motion.data(), ctx->motion_xf.p, (size_t)n * 48, hipMemcpyDeviceToHost) != hipSuccess))
      return lost(fail(ctx, STHIP_ERR_HIP, call + "reading the resident matrices failed"));
    if ((rc = update_transforms_host(ctx, call, xf.data(), inv.data(), ctx->motion_xf.p ? motion.data() : nullptr, n, nullptr)) != STHIP_OK) return lost(rc);
  }
  local.device_ms = 0;
  (void)hipEventElapsedTime(&local.device_ms, ctx->edit_ev[0], ctx->edit_ev[1]);
  local.device_ms += build_ms;
  local.call_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (info) *info = local;
  return STHIP_OK;
}

// The device builder of sthip_scene_set_transforms (top_level.hip). `xf` / `inv` / `motion` are device memory here.
static int set_transforms_device(sthip_ctx* ctx, const std::string& call, const sthip_TransformData* xf, const sthip_TransformData* inv, const sthip_TransformData* motion, bool derive_motion,
                                 bool host_mirrors_follow, const sthip_TransformData* host_xf, const sthip_TransformData* host_inv, const sthip_TransformData* host_motion, sthip_transforms_info* info) {
  const uint32_t n = ctx->instance_count, m = (uint32_t)ctx->top.entries.size();
  std::string err;
  // ---- reserve ----
  if (!ctx->top_level) ctx->top_level = sthip::device_top_level_create();
  if (!ctx->top_level_static_valid) {
    if (!sthip::top_level_set_static(ctx->top_level, ctx->top.merged.data(), n, ctx->top.obj_box.data(), m, ctx->stream, err)) return fail(ctx, STHIP_ERR_HIP, call + err);
    ctx->top_level_static_valid = true;
  }
  // ---- frames in flight still read the resident arrays; the work below reads them too (entries, the previous transforms) ----
  if (const int rc = quiesce(ctx); rc != STHIP_OK) return rc;
  sthip::TopLevelInputs in;
  in.xf = xf;
  in.inv = inv;
  in.motion = motion;
  in.derive_motion = derive_motion;
  in.instance_count = n;
  in.resident_xf = ctx->xf.p;
  in.entries = ctx->entries.p;
  in.entry_count = m;
  in.volumes = ctx->volumes.p;
  in.volume_count = (uint32_t)std::min<size_t>(ctx->volumes.n, ctx->top.volumes.size());
  memcpy(in.merged_box, ctx->top.merged_box, sizeof(in.merged_box));
  in.blas_nodes = ctx->top.blas_nodes;
  const bool lone_identity = m == 1 && ctx->top.entries[0].identity == TLAS_ENTRY_IDENTITY;
  in.build_tree = m >= 1 && !lone_identity;
  sthip::TopLevelResult res{};
  float gpu_ms = 0;
  if (!sthip::top_level_build(ctx->top_level, in, ctx->stream, res, gpu_ms, err)) return fail(ctx, STHIP_ERR_HIP, call + err);
  // ---- everything that can be refused is decided here, from the one read-back; nothing resident has been written ----
  if (res.flags & TL_FLAG_SINGULAR)
    return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, call + "the transform of instance " + std::to_string(res.first_bad) + " (or a later one) has no inverse: its determinant is 0 or not finite");
  if (res.flags & TL_FLAG_MERGED_MOVED) {
    if (ctx->kept.valid && ctx->kept.instances.size() == n) {  // the matrices come to the host and the scene is built again, as the host path does
      std::vector<sthip_TransformData> hx(n), hi(n), hm(n);
      DevBuf<sthip_TransformData> tmp;  // (the staging holds the call's three arrays, derived ones included)
      HIP_TRY(ctx, tmp.ensure((size_t)3 * n));
      if (!sthip::top_level_install(ctx->top_level, tmp.p, tmp.p + n, tmp.p + 2 * (size_t)n, nullptr, nullptr, ctx->stream, err)) return fail(ctx, STHIP_ERR_HIP, call + err);
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      HIP_TRY(ctx, hipMemcpy(hx.data(), tmp.p, (size_t)n * 48, hipMemcpyDeviceToHost));
      HIP_TRY(ctx, hipMemcpy(hi.data(), tmp.p + n, (size_t)n * 48, hipMemcpyDeviceToHost));
      HIP_TRY(ctx, hipMemcpy(hm.data(), tmp.p + 2 * (size_t)n, (size_t)n * 48, hipMemcpyDeviceToHost));
      ctx->kept.set_transforms(hx.data(), hi.data(), hm.data(), n);
      ctx->host_transforms_stale = false;
      ctx->stats.full_rebuilds++;
      if (info) info->rebuilt = 1;
      return upload_kept_scene(ctx);
    }
    return fail(ctx, STHIP_ERR_UNSUPPORTED, call + "an instance of the merged world-space mesh (identity transform at upload) moved: upload the scene again");
  }
  if (res.flags & TL_FLAG_BOX) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, call + "the world box of top-level entry " + std::to_string(res.first_bad) + " (or a later one) is not finite");
  const uint32_t tlas_count = in.build_tree ? (m >= 2 ? m - 1 : 1) : 0;
  const uint32_t tlas_depth = tlas_count ? res.height + 1 : 0;
  const uint32_t stack_depth = tlas_depth + ctx->top.blas_depth + 3;
  if (stack_depth > STHIP_MAX_STACK_DEPTH) return fail(ctx, STHIP_ERR_UNSUPPORTED, call + "the new top level is too deep for the traversal stack");
  if ((size_t)ctx->top.blas_nodes + tlas_count > ctx->nodes.n) return fail(ctx, STHIP_ERR_UNSUPPORTED, call + "the new top level does not fit: upload the scene again");
  // ---- install ----
  if (!sthip::top_level_install(ctx->top_level, ctx->xf.p, ctx->inv_xf.p, ctx->motion_xf.p, ctx->entries.p, ctx->nodes.p + ctx->top.blas_nodes, ctx->stream, err)) return fail(ctx, STHIP_ERR_HIP, call + err);
  float center[3] = {ctx->bvh.scene_cx, ctx->bvh.scene_cy, ctx->bvh.scene_cz}, radius = ctx->bvh.scene_radius;
  {
    float lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
      lo[a] = sthip::top_level_ord2f(res.box[a]);
      hi[a] = sthip::top_level_ord2f(res.box[3 + a]);
    }
    if (m && lo[0] <= hi[0]) {  // (rebuild_top_level's formulas)
      for (int a = 0; a < 3; a++) center[a] = 0.5f * (lo[a] + hi[a]);
      radius = 0.5f * sqrtf((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
    }
  }
  uint32_t root_ref = BVH_INVALID_REF, top_is_world = 1;
  if (lone_identity) {
    root_ref = ctx->top.entries[0].root;
  } else if (m) {
    root_ref = ctx->top.blas_nodes;  // (node 0 of a radix tree is its root; the wrapped leaf is the only node)
    top_is_world = 0;
  }
  // the host's mirrors: they follow at once where the call's arrays are host memory and nothing was derived, else lazily
  if (host_mirrors_follow) {
    if (ctx->kept.valid && ctx->kept.instances.size() == n) ctx->kept.set_transforms(host_xf, host_inv, host_motion, n);
    for (TlasEntry& e : ctx->top.entries)
      if (e.identity != TLAS_ENTRY_IDENTITY && e.id_bits < n) memcpy(e.inv, &host_inv[e.id_bits], 48);
    ctx->host_transforms_stale = false;
  } else {
    ctx->host_transforms_stale = true;
  }
  // layouts whose top level the host makes from host nodes: the new binary nodes come back once, and the entries' inverses
  std::vector<BvhNode> tlas;
  if (ctx->bvh.wide8_nodes || !ctx->wide8_host.empty() || ctx->use_treetop || ctx->nodes_host.n) {
    tlas.resize(tlas_count);
    if (!sthip::top_level_read_nodes(ctx->top_level, tlas.data(), tlas_count, ctx->stream, err)) return fail(ctx, STHIP_ERR_HIP, call + err);
    const int rc = sync_kept_transforms(ctx);
    if (rc != STHIP_OK) return rc;
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the collapse and the copies of the layouts go through other queues)
  const float wide_before = ctx->stats.bvh_build_gpu_ms;
  const int rc = finish_top_level(ctx, tlas.empty() ? nullptr : tlas.data(), tlas_count, root_ref, top_is_world, stack_depth, center, radius);
  if (info) {
    info->device_ms = gpu_ms + (ctx->stats.bvh_build_gpu_ms - wide_before);
    info->top_level_nodes = tlas_count;
    info->top_level_depth = tlas_depth;
    info->builder_used = 1;
  }
  return rc;
}

int sthip_scene_set_transforms(sthip_ctx* ctx, const sthip_transforms_desc* d, uint32_t struct_size, sthip_transforms_info* info) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  const auto t0 = std::chrono::steady_clock::now();
  const std::string call = "sthip_scene_set_transforms: ";
  if (info) memset(info, 0, sizeof(*info));
  if (!ctx->has_scene) return fail(ctx, STHIP_ERR_NO_SCENE, "sthip_scene_set_transforms before sthip_scene_upload");
  if (!d) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, call + "desc is NULL");
  if (struct_size != sizeof(sthip_transforms_desc)) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, call + "struct_size is not sizeof(sthip_transforms_desc)");
  if (!d->transforms) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, call + "transforms is NULL");
  if (d->derive_motion && d->motion_transforms) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, call + "derive_motion and motion_transforms exclude each other");
  if (d->top_level > 1 || d->device_ptr > 1 || d->derive_motion > 1) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, call + "top_level, device_ptr and derive_motion are 0 or 1");
  if (d->instance_count != ctx->instance_count) return fail(ctx, STHIP_ERR_UNSUPPORTED, call + "the instance count changed: upload the scene again");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint32_t n = d->instance_count;
  int rc = STHIP_OK;
  auto finish = [&](int code) {
    if (info) info->total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return code;
  };
  if (d->top_level == 1 && ctx->top.entries.size() > 0xFFFFu)  // (an upload takes fewer: the keys of top_level.hip hold a 16-bit entry index)
    return fail(ctx, STHIP_ERR_UNSUPPORTED, call + "more top-level entries than the device builder's keys can index");
  if (d->top_level == 1) {
    ctx->scene_serial++;
    const sthip_TransformData *xf = d->transforms, *inv = d->inverse_transforms, *motion = d->motion_transforms;
    DevBuf<sthip_TransformData> up;  // host arrays: they go up once, into a staging of the call
    if (!d->device_ptr) {
      HIP_TRY(ctx, up.ensure(std::max<size_t>(1, (size_t)3 * n)));
      HIP_TRY(ctx, hipMemcpyAsync(up.p, xf, (size_t)n * 48, hipMemcpyHostToDevice, ctx->stream));
      xf = up.p;
      if (inv) {
        HIP_TRY(ctx, hipMemcpyAsync(up.p + n, inv, (size_t)n * 48, hipMemcpyHostToDevice, ctx->stream));
        inv = up.p + n;
      }
      if (motion) {
        HIP_TRY(ctx, hipMemcpyAsync(up.p + 2 * (size_t)n, motion, (size_t)n * 48, hipMemcpyHostToDevice, ctx->stream));
        motion = up.p + 2 * (size_t)n;
      }
    }
    const bool follow = !d->device_ptr && d->inverse_transforms && !d->derive_motion;
    rc = set_transforms_device(ctx, call, xf, inv, motion, d->derive_motion != 0, follow, d->transforms, d->inverse_transforms, d->motion_transforms, info);
    const hipError_t e = hipStreamSynchronize(ctx->stream);  // (`up` goes out of scope)
    if (rc == STHIP_OK && e != hipSuccess) rc = fail(ctx, STHIP_ERR_HIP, call + hipGetErrorString(e));
    return finish(rc);
  }
  // ---- the host builder: the matrices as host arrays (copied back once; derived with the same arithmetic), then today's path ----
  std::vector<sthip_TransformData> hx, hi, hm;
  const sthip_TransformData *xf = d->transforms, *inv = d->inverse_transforms, *motion = d->motion_transforms;
  if (d->device_ptr) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    hx.resize(n);
    HIP_TRY(ctx, hipMemcpy(hx.data(), xf, (size_t)n * 48, hipMemcpyDeviceToHost));
    xf = hx.data();
    if (inv) {
      hi.resize(n);
      HIP_TRY(ctx, hipMemcpy(hi.data(), inv, (size_t)n * 48, hipMemcpyDeviceToHost));
      inv = hi.data();
    }
    if (motion) {
      hm.resize(n);
      HIP_TRY(ctx, hipMemcpy(hm.data(), motion, (size_t)n * 48, hipMemcpyDeviceToHost));
      motion = hm.data();
    }
  }
  if (!inv) {
    hi.resize(n);
    for (uint32_t i = 0; i < n; i++)
      if (!sthip::derive_inverse(&xf[i].m[0][0], &hi[i].m[0][0]))
        return finish(fail(ctx, STHIP_ERR_INVALID_ARGUMENT, call + "the transform of instance " + std::to_string(i) + " has no inverse: its determinant is 0 or not finite"));
    inv = hi.data();
  }
  if (d->derive_motion) {
    std::vector<sthip_TransformData> prev(n);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (n) HIP_TRY(ctx, hipMemcpy(prev.data(), ctx->xf.p, (size_t)n * 48, hipMemcpyDeviceToHost));
    hm.resize(n);
    for (uint32_t i = 0; i < n; i++) sthip::derive_motion(&prev[i].m[0][0], &inv[i].m[0][0], &hm[i].m[0][0]);
    motion = hm.data();
  }
  rc = update_transforms_host(ctx, call, xf, inv, motion, n, info);
  return finish(rc);
}

int sthip_scene_read_transforms(sthip_ctx* ctx, uint32_t first, uint32_t count, sthip_TransformData* xf, sthip_TransformData* inv, sthip_TransformData* motion) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  if (!ctx->has_scene) return fail(ctx, STHIP_ERR_NO_SCENE, "sthip_scene_read_transforms before sthip_scene_upload");
  if ((uint64_t)first + count > ctx->instance_count) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_scene_read_transforms: the range ends past the instance count of the resident scene");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (!count) return STHIP_OK;
  if (xf) HIP_TRY(ctx, hipMemcpy(xf, ctx->xf.p + first, (size_t)count * 48, hipMemcpyDeviceToHost));
  if (inv) HIP_TRY(ctx, hipMemcpy(inv, ctx->inv_xf.p + first, (size_t)count * 48, hipMemcpyDeviceToHost));
  if (motion) HIP_TRY(ctx, hipMemcpy(motion, ctx->motion_xf.p + first, (size_t)count * 48, hipMemcpyDeviceToHost));
  return STHIP_OK;
}

int sthip_scene_read_top_level(sthip_ctx* ctx, float* entry_boxes, sthip_top_node* nodes, uint32_t node_capacity, uint32_t* entry_count, uint32_t* node_count, uint32_t* root, float center_radius[4]) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  const std::string call = "sthip_scene_read_top_level: ";
  if (!ctx->has_scene) return fail(ctx, STHIP_ERR_NO_SCENE, "sthip_scene_read_top_level before sthip_scene_upload");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint32_t n = ctx->instance_count, m = (uint32_t)ctx->top.entries.size(), blas_nodes = ctx->top.blas_nodes;
  const uint32_t count = ctx->bvh.top_is_world_blas ? 0u : (uint32_t)(ctx->bvh_nodes - blas_nodes);
  if (entry_count) *entry_count = m;
  if (node_count) *node_count = count;
  if (root) *root = ctx->bvh.top_is_world_blas ? 0xFFFFFFFFu : ctx->bvh.root_ref - blas_nodes;
  if (center_radius) {
    center_radius[0] = ctx->bvh.scene_cx;
    center_radius[1] = ctx->bvh.scene_cy;
    center_radius[2] = ctx->bvh.scene_cz;
    center_radius[3] = ctx->bvh.scene_radius;
  }
  if (nodes && node_capacity < count) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, call + "node_capacity is smaller than the node count");
  std::string err;
  if (entry_boxes && m) {  // the boxes of the resident matrices, by the kernel every device build uses
    if (!ctx->top_level) ctx->top_level = sthip::device_top_level_create();
    if (!ctx->top_level_static_valid) {
      if (!sthip::top_level_set_static(ctx->top_level, ctx->top.merged.data(), n, ctx->top.obj_box.data(), m, ctx->stream, err)) return fail(ctx, STHIP_ERR_HIP, call + err);
      ctx->top_level_static_valid = true;
    }
    sthip::TopLevelInputs in;
    in.xf = ctx->xf.p;
    in.inv = ctx->inv_xf.p;
    in.motion = ctx->motion_xf.p;
    in.instance_count = n;
    in.resident_xf = ctx->xf.p;
    in.entries = ctx->entries.p;
    in.entry_count = m;
    in.volumes = ctx->volumes.p;
    in.volume_count = (uint32_t)std::min<size_t>(ctx->volumes.n, ctx->top.volumes.size());
    memcpy(in.merged_box, ctx->top.merged_box, sizeof(in.merged_box));
    in.blas_nodes = blas_nodes;
    in.build_tree = false;
    sthip::TopLevelResult res{};
    float ms = 0;
    if (!sthip::top_level_build(ctx->top_level, in, ctx->stream, res, ms, err)) return fail(ctx, STHIP_ERR_HIP, call + err);
    if (!sthip::top_level_read_boxes(ctx->top_level, entry_boxes, m, ctx->stream, err)) return fail(ctx, STHIP_ERR_HIP, call + err);
  }
  if (nodes && count) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<BvhNodeSlot> slots(count);
    HIP_TRY(ctx, hipMemcpy(slots.data(), ctx->nodes.p + blas_nodes, (size_t)count * sizeof(BvhNodeSlot), hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < count; k++) {
      // a plane with the reference byte in its low mantissa byte: whatever that byte holds the plane lies outside the box, so
      // the byte is pushed outward here (a lower plane to its least value, an upper plane to its greatest)
      uint32_t w[8], ref[2] = {0, 0};
      memcpy(w, slots[k].n.n0xy, 16);
      memcpy(w + 4, slots[k].n.n1xy, 16);
      float plane[2][6];
      for (int c = 0; c < 2; c++) {
        for (int j = 0; j < 4; j++) {
          const uint32_t u = w[4 * c + j];
          ref[c] |= (u & 0xFFu) << (8 * j);
          const bool upper = (j & 1) != 0, negative = (u >> 31) != 0;
          const uint32_t out = (upper != negative) ? (u | 0xFFu) : (u & ~0xFFu);
          memcpy(&plane[c][j], &out, 4);
        }
        plane[c][4] = slots[k].n.nz[2 * c];
        plane[c][5] = slots[k].n.nz[2 * c + 1];
      }
      sthip_top_node& o = nodes[k];
      for (int a = 0; a < 3; a++) {
        o.lo[a] = std::min(plane[0][2 * a], plane[1][2 * a]);
        o.hi[a] = std::max(plane[0][2 * a + 1], plane[1][2 * a + 1]);
      }
      uint32_t* child[2] = {&o.child0, &o.child1};
      for (int c = 0; c < 2; c++) *child[c] = (ref[c] & BVH_LEAF_BIT) ? (0x80000000u | (ref[c] & 0xFFFFu)) : ref[c] - blas_nodes;
    }
  }
  return STHIP_OK;
}

// Where the new vertex records of a refit come from: a range of host records that goes up (sthip_scene_update_vertices), or
// the resident rigs in the pose an animate call staged, written on the device (sthip_scene_animate: `vertices` is NULL), or
// streams on the device that are packed into the range there (sthip_scene_set_vertices: `streams`)
struct VertexSource {
  const char* call;  // the entry point, for messages
  const sthip_PackedVertexData* vertices;
  uint32_t first_vertex, vertex_count;
  const sthip::VertexStreams* streams = nullptr;
  bool recompute_normals = false;
  bool streamed() const { return streams != nullptr; }
  bool posed() const { return vertices == nullptr && !streams; }
  bool on_device() const { return vertices == nullptr; }  // the device writes the records: the kept scene falls behind
};

// The kernels of sthip_scene_set_vertices: the pack, then the normals of the range. From the first launch on the kept
// vertices of the range are behind the device's.
static int write_vertex_streams(sthip_ctx* ctx, const VertexSource& src) {
  if (ctx->kept.valid && src.vertex_count) {
    ctx->kept.vertices_written(src.first_vertex, src.vertex_count);  // (one entry per range, however often it is written)
    ctx->kept.stale_vertices.emplace_back(src.first_vertex, src.first_vertex + src.vertex_count);
  }
  std::string err;
  StageTimer times(vertex_times_file(), true, 4);  // (measurement only: sthip.h)
  HIP_TRY(ctx, hipEventRecord(ctx->edit_ev[0], ctx->stream));
  times.mark(0, ctx->stream);
  if (!sthip::pack_vertices_launch(ctx->vertices.p, *src.streams, ctx->stream, err)) return fail(ctx, STHIP_ERR_HIP, std::string(src.call) + ": " + err);
  times.mark(1, ctx->stream);
  if (src.recompute_normals &&
      !sthip::vertex_normals_launch(ctx->adjacency, ctx->vertices.p, ctx->vertex_count, ctx->indices.p, ctx->indices_bytes, src.first_vertex, src.vertex_count, ctx->stream,
                                    times.on ? times.ev[2] : nullptr, err))
    return fail(ctx, STHIP_ERR_HIP, std::string(src.call) + ": " + err);
  if (!src.recompute_normals) times.mark(2, ctx->stream);
  times.mark(3, ctx->stream);
  HIP_TRY(ctx, hipEventRecord(ctx->edit_ev[1], ctx->stream));
  if (times.on) {
    static const char* const names[3] = {"k_pack_vertices_ms", "k_face_vectors_ms", "k_vertex_normals_ms"};
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    times.write("\"call\": \"" + std::string(src.call) + "\", \"vertices\": " + std::to_string(src.vertex_count) + ", \"recompute_normals\": " + (src.recompute_normals ? "1" : "0"), names);
  }
  return STHIP_OK;
}

// The layouts a vertex update does not refit: they are built again from the kept scene
static bool layout_not_refitted(const sthip_ctx* ctx) { return ctx->embedded_resident || ctx->use_treetop || ctx->bvh.top_count || ctx->bvh.wide8_nodes || !ctx->wide8_host.empty(); }

// The part of a vertex update that changes the resident scene: the vertex range goes up or the rigs are posed, the leaf
// triangles are gathered again, the bottom levels refitted and everything an upload derives from the meshes' bounds made again.
// A failure in here leaves the scene half changed; the caller repairs that.
static int refit_resident_scene(sthip_ctx* ctx, const VertexSource& src, bool kept, const sthip_TransformData* xf, const sthip_TransformData* inv, sthip::RefitResult& res, float& wide_ms) {
  std::string err;
  const std::string call = std::string(src.call) + ": ";
  const uint32_t n = ctx->instance_count;
  const std::vector<uint32_t>& root_of_entry = ctx->refit_root_of_entry;
  if (src.posed()) {
    const int rc = pose_rigs(ctx, src.call);
    if (rc != STHIP_OK) return rc;
  } else if (src.streamed()) {
    const int rc = write_vertex_streams(ctx, src);
    if (rc != STHIP_OK) return rc;
  } else if (src.vertex_count) {
    const sthip_PackedVertexData* vertices = src.vertices;
    const uint32_t first_vertex = src.first_vertex, vertex_count = src.vertex_count;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->vertices.p + first_vertex, vertices, (size_t)vertex_count * sizeof(sthip_PackedVertexData), hipMemcpyHostToDevice, ctx->stream));
    if (kept && vertices != ctx->kept.vertices.data() + first_vertex) memcpy(ctx->kept.vertices.data() + first_vertex, vertices, (size_t)vertex_count * sizeof(sthip_PackedVertexData));
    if (kept) ctx->kept.vertices_written(first_vertex, vertex_count);
  }
  ctx->reuse_grids_valid = false;
  ctx->nodes_host.n = 0;  // (no layout that reads the host copy of the nodes comes this way; it must not outlive the boxes it holds)
  drop_leaf_pairs(ctx);   // (new positions go into BvhTri only; the wide form is collapsed again below)
  if (!sthip::refit_gather(ctx->refit, ctx->tris.p, (uint32_t)ctx->bvh_tris, ctx->vertices.p, ctx->vertex_count, ctx->indices.p, ctx->indices_bytes, ctx->stream, err))
    return fail(ctx, STHIP_ERR_HIP, call + err);
  if (ctx->bvh_tris && ctx->vertex_count) {
    const int rc = launch_fill_tri_shade(ctx, (size_t)ctx->bvh_tris, nullptr);
    if (rc != STHIP_OK) return rc;
  }
  std::vector<uint32_t> emitter_instances;
  for (uint32_t k = 0; k < ctx->emitter_count && k < ctx->emitters_host.size(); k++) emitter_instances.push_back(ctx->emitters_host[k].instance);
  if (!sthip::refit_boxes(ctx->refit, ctx->nodes.p, ctx->tris.p, (uint32_t)ctx->bvh_tris, ctx->instances.p, emitter_instances, ctx->vertices.p, ctx->vertex_count, ctx->indices.p, ctx->indices_bytes,
                          ctx->stream, res, err))
    return fail(ctx, STHIP_ERR_HIP, call + err);
  // what an upload derives from the meshes' bounds (bvh_build.cpp), with its arithmetic, from the roots' exact boxes
  ctx->top_level_static_valid = false;  // (top_level.hip keeps the object boxes on the device: they change here)
  sthip::TopLevelState next = ctx->top;
  for (size_t k = 0; k < next.entries.size(); k++) {
    if (root_of_entry[k] == BVH_INVALID_REF) continue;
    const float* lo = &res.root_boxes[8 * (size_t)root_of_entry[k]];
    const float* hi = lo + 4;
    if (!(lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2])) continue;
    TlasEntry& e = next.entries[k];
    for (int a = 0; a < 3; a++) e.center[a] = 0.5f * (lo[a] + hi[a]);
    e.radius = 0.5f * sqrtf((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
    if (e.identity == TLAS_ENTRY_IDENTITY) {
      memcpy(next.merged_box, lo, 12);
      memcpy(next.merged_box + 3, hi, 12);
    } else {
      memcpy(&next.obj_box[6 * k], lo, 12);
      memcpy(&next.obj_box[6 * k + 3], hi, 12);
    }
  }
  if (!emitter_instances.empty()) {
    bool usable = true;
    for (size_t k = 0; k < emitter_instances.size(); k++) {
      EmitterBounds& b = ctx->emitters_host[k];
      memcpy(b.lo, &res.emitter_boxes[8 * k], 12);
      memcpy(b.hi, &res.emitter_boxes[8 * k + 4], 12);
      if (!(b.lo[0] <= b.hi[0]) || !sthip::pad_emitter_bounds(b)) usable = false;
    }
    if (usable) {
      HIP_TRY(ctx, hipMemcpy(ctx->emitters.p, ctx->emitters_host.data(), emitter_instances.size() * sizeof(EmitterBounds), hipMemcpyHostToDevice));
    } else {  // (no bounds to aim at: every last ray is traced)
      ctx->emitter_count = 0;
      ctx->emitters_host.clear();
    }
  }
  std::vector<BvhNode> tlas;
  uint32_t root_ref = 0, top_is_world = 1, stack_depth = 4;
  float center[3] = {ctx->bvh.scene_cx, ctx->bvh.scene_cy, ctx->bvh.scene_cz}, radius = ctx->bvh.scene_radius;
  if (!sthip::rebuild_top_level(next, xf, inv, n, tlas, root_ref, top_is_world, stack_depth, center, radius, err)) return fail(ctx, STHIP_ERR_UNSUPPORTED, call + err);
  if (stack_depth > STHIP_MAX_STACK_DEPTH) return fail(ctx, STHIP_ERR_UNSUPPORTED, call + "the new top level is too deep for the traversal stack");
  if ((size_t)next.blas_nodes + tlas.size() > ctx->nodes.n) return fail(ctx, STHIP_ERR_UNSUPPORTED, call + "the new top level does not fit");
  const float wide_ms_before = ctx->stats.bvh_build_gpu_ms;
  const int rc = install_top_level(ctx, next, tlas, root_ref, top_is_world, stack_depth, center, radius);
  wide_ms = ctx->stats.bvh_build_gpu_ms - wide_ms_before;
  return rc;
}

// sthip.h, for both sources of new vertices. The default layout is refitted where it lies (refit.hip); the layouts that keep
// more than the node and triangle arrays of the tree (leaf triangles inside the node array, a treetop selected from a host
// copy of the nodes, the 8-wide form with its permuted triangles) are built again from the kept scene.
static int update_resident_vertices(sthip_ctx* ctx, const VertexSource& src, sthip_refit_info* info, std::chrono::steady_clock::time_point t0) {
  const std::string call = std::string(src.call) + ": ";
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ctx->scene_serial++;  // (first_hits.h: sthip_scene_update_vertices and sthip_scene_animate both come this way)
  const bool kept = ctx->kept.valid && ctx->kept.vertices.size() == ctx->vertex_count;
  auto rebuild_from_kept = [&]() {  // (the kept vertices hold the new range already, or get the posed ranges back from the device there)
    ctx->stats.full_rebuilds++;
    const int rc = upload_kept_scene(ctx);
    if (info) {
      info->rebuilt = 1;
      info->device_ms = ctx->stats.bvh_build_gpu_ms;
      info->total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return rc;
  };
  if (src.on_device())
    if (const int rc = make_edit_events(ctx); rc != STHIP_OK) return rc;
  if (layout_not_refitted(ctx)) {
    if (!kept) return fail(ctx, STHIP_ERR_UNSUPPORTED, call + "this layout (embed_leaves, treetop, wide_bvh = 3) is not refitted and no scene was kept (keep_scene = 0): upload the scene again");
    if (src.on_device()) {  // the kernels, then the rebuild reads their ranges back
      if (const int rc = quiesce(ctx); rc != STHIP_OK) return rc;
      const int rc = src.posed() ? pose_rigs(ctx, src.call) : write_vertex_streams(ctx, src);
      if (rc != STHIP_OK) return rc;
    } else if (src.vertex_count) {
      const int rc = sync_kept_vertices(ctx);  // (before the host's records go in: they are the newer ones)
      if (rc != STHIP_OK) return rc;
      memcpy(ctx->kept.vertices.data() + src.first_vertex, src.vertices, (size_t)src.vertex_count * sizeof(sthip_PackedVertexData));
    }
    return rebuild_from_kept();
  }
  // everything that can fail for want of memory happens before anything of the resident scene changes
  if (!ctx->refit_roots_valid || ctx->refit_root_of_entry.size() != ctx->top.entries.size()) {
    std::unordered_map<uint32_t, uint32_t> place;  // (instances that share a mesh share its root)
    ctx->refit_roots.clear();
    ctx->refit_root_of_entry.assign(ctx->top.entries.size(), BVH_INVALID_REF);
    for (size_t k = 0; k < ctx->top.entries.size(); k++) {
      const TlasEntry& e = ctx->top.entries[k];
      if ((e.identity != TLAS_ENTRY_IDENTITY && e.identity != TLAS_ENTRY_TRANSFORMED) || (e.root & BVH_LEAF_BIT) || e.root >= ctx->top.blas_nodes) continue;
      const auto at = place.emplace(e.root, (uint32_t)ctx->refit_roots.size());
      if (at.second) ctx->refit_roots.push_back(e.root);
      ctx->refit_root_of_entry[k] = at.first->second;
    }
    ctx->refit_roots_valid = true;
  }
  if (!ctx->refit) ctx->refit = sthip::device_refit_create();
  // frames in flight still read the old triangles and boxes (sthip_render_async: their copies too, so that their tickets are complete)
  if (const int rc = quiesce(ctx); rc != STHIP_OK) return rc;
  std::string err;
  if (!sthip::refit_prepare(ctx->refit, ctx->nodes.p, ctx->top.blas_nodes, ctx->refit_roots, ctx->top.blas_depth, ctx->tris.p, (uint32_t)ctx->bvh_tris, STHIP_MAX_EMITTER_BOUNDS, ctx->stream, err))
    return fail(ctx, STHIP_ERR_HIP, call + err);
  // the instances' transforms, for the top level: the kept scene has them (sthip_scene_update_transforms keeps it current);
  // without one they are read back from the device
  const uint32_t n = ctx->instance_count;
  {  // (a device-pointer call of sthip_scene_set_transforms left the kept matrices behind the device's)
    const int rc = sync_kept_transforms(ctx);
    if (rc != STHIP_OK) return rc;
  }
  std::vector<sthip_TransformData> xf_read, inv_read;
  const sthip_TransformData *xf = nullptr, *inv = nullptr;
  if (ctx->kept.valid && ctx->kept.xf.size() == n && ctx->kept.inv.size() == n) {
    xf = ctx->kept.xf.data();
    inv = ctx->kept.inv.data();
  } else {
    xf_read.resize(n);
    inv_read.resize(n);
    HIP_TRY(ctx, hipMemcpy(xf_read.data(), ctx->xf.p, (size_t)n * 48, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(inv_read.data(), ctx->inv_xf.p, (size_t)n * 48, hipMemcpyDeviceToHost));
    xf = xf_read.data();
    inv = inv_read.data();
  }
  // ---- from here on the resident scene changes ----
  sthip::RefitResult res;
  float wide_ms = 0;
  const int rc = refit_resident_scene(ctx, src, kept, xf, inv, res, wide_ms);
  if (rc != STHIP_OK) {
    // New triangles under old entries or an old top level would miss hits without a word. With a kept scene (it holds the new
    // vertices by now, or reads the posed ones back) the scene is built again, as for the layouts above; without one no scene
    // is resident any more, as after a failed sthip_scene_upload, and every call that needs one says so until the host uploads again.
    if (kept) return rebuild_from_kept();
    const std::string why = ctx->error;
    ctx->has_scene = false;
    sthip::device_refit_invalidate(ctx->refit);
    sthip::device_vertex_adjacency_invalidate(ctx->adjacency);
    ctx->refit_roots_valid = false;
    return fail(ctx, rc, why + " (the resident scene was dropped half changed: upload the scene again)");
  }
  if (info) {
    float pose_ms = 0;  // (refit_boxes has waited for the stream: the events around k_animate have been reached)
    if (src.on_device()) (void)hipEventElapsedTime(&pose_ms, ctx->edit_ev[0], ctx->edit_ev[1]);
    info->device_ms = pose_ms + res.gpu_ms + wide_ms;
    info->sah_cost = (float)res.sah_cost;
    info->sah_cost_at_build = (float)res.sah_cost_at_build;
    info->rebuilt = 0;
    info->total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return STHIP_OK;
}

int sthip_scene_update_vertices(sthip_ctx* ctx, const sthip_PackedVertexData* vertices, uint32_t first_vertex, uint32_t vertex_count, sthip_refit_info* info) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  const auto t0 = std::chrono::steady_clock::now();
  if (info) memset(info, 0, sizeof(*info));
  if (!ctx->has_scene) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_scene_update_vertices before sthip_scene_upload");
  if (!vertices) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_scene_update_vertices: vertices is NULL");
  if ((uint64_t)first_vertex + vertex_count > ctx->vertex_count)
    return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_scene_update_vertices: the range ends past the vertex_count of the uploaded scene");
  return update_resident_vertices(ctx, VertexSource{"sthip_scene_update_vertices", vertices, first_vertex, vertex_count}, info, t0);
}

// sthip.h: refused on the host (scene_prepare.cpp), then everything that needs memory is made — the staging of host streams,
// the adjacency of the resident topology at the first call that asks for normals — and from there on the call is a vertex
// update whose records are written by k_pack_vertices (and k_vertex_normals) instead of coming up from the host.
int sthip_scene_set_vertices(sthip_ctx* ctx, const sthip_vertex_streams* d, sthip_refit_info* info) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  const auto t0 = std::chrono::steady_clock::now();
  if (info) memset(info, 0, sizeof(*info));
  const std::string call = "sthip_scene_set_vertices: ";
  {
    int code = STHIP_OK;
    std::string message;
    if (!sthip::check_vertex_streams(ctx->has_scene, ctx->vertex_count, d, code, message)) return fail(ctx, code, message);
  }
  if (!d->vertex_count) return STHIP_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (layout_not_refitted(ctx) && !(ctx->kept.valid && ctx->kept.vertices.size() == ctx->vertex_count))  // (before anything is made for the call)
    return fail(ctx, STHIP_ERR_UNSUPPORTED, call + "this layout (embed_leaves, treetop, wide_bvh = 3) is not refitted and no scene was kept (keep_scene = 0): upload the scene again");
  sthip::VertexStreams s;
  s.positions = d->positions;
  s.normals = d->normals;
  s.texcoords = d->texcoords;
  s.position_stride = d->position_stride;
  s.normal_stride = d->normal_stride;
  s.texcoord_stride = d->texcoord_stride;
  s.first_vertex = d->first_vertex;
  s.vertex_count = d->vertex_count;
  if (!d->device_ptr) {  // the spans of the host streams go up as they are (strides and all): one code path on the device
    const void** stream_of[3] = {&s.positions, &s.normals, &s.texcoords};
    const uint32_t strides[3] = {s.position_stride, s.normal_stride, s.texcoord_stride}, elements[3] = {12, 12, 8};
    size_t at[3] = {0, 0, 0}, span[3] = {0, 0, 0}, total = 0;
    for (int k = 0; k < 3; k++) {
      if (!*stream_of[k]) continue;
      span[k] = (size_t)(d->vertex_count - 1) * strides[k] + elements[k];
      at[k] = total;
      total += (span[k] + 15) & ~(size_t)15;
    }
    HIP_TRY(ctx, ctx->stream_staging.ensure(total));
    for (int k = 0; k < 3; k++) {
      if (!*stream_of[k]) continue;
      HIP_TRY(ctx, hipMemcpyAsync(ctx->stream_staging.p + at[k], *stream_of[k], span[k], hipMemcpyHostToDevice, ctx->stream));
      *stream_of[k] = ctx->stream_staging.p + at[k];
    }
  }
  if (d->recompute_normals) {
    if (!ctx->adjacency) ctx->adjacency = sthip::device_vertex_adjacency_create();
    if (!sthip::vertex_adjacency_valid(ctx->adjacency)) {
      // the instances say which meshes there are: the kept scene has them; without one they are read back from the device
      std::vector<sthip_InstanceData> read;
      const sthip_InstanceData* instances = ctx->kept.valid && ctx->kept.instances.size() == ctx->instance_count ? ctx->kept.instances.data() : nullptr;
      if (!instances) {
        read.resize(ctx->instance_count);
        if (ctx->instance_count) HIP_TRY(ctx, hipMemcpy(read.data(), ctx->instances.p, (size_t)ctx->instance_count * sizeof(sthip_InstanceData), hipMemcpyDeviceToHost));
        instances = read.data();
      }
      std::string err;
      bool built = false;
      if (!sthip::vertex_adjacency_prepare(ctx->adjacency, sthip::list_vertex_meshes(instances, ctx->instance_count), ctx->indices.p, ctx->indices_bytes, ctx->vertex_count, ctx->stream, built, err))
        return fail(ctx, STHIP_ERR_HIP, call + err);
    }
  }
  VertexSource src{"sthip_scene_set_vertices", nullptr, d->first_vertex, d->vertex_count};
  src.streams = &s;
  src.recompute_normals = d->recompute_normals != 0;
  return update_resident_vertices(ctx, src, info, t0);
}

// sthip.h: validated on the host, then the rest poses are taken on the device and targets and weights go up once. Everything is
// made beside the resident rigs and swapped in at the end, so a refused or failed call leaves them as they were.
int sthip_scene_set_rigs(sthip_ctx* ctx, const sthip_rig_desc* rigs, uint32_t rig_count) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  const std::string call = "sthip_scene_set_rigs: ";
  if (!ctx->has_scene) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_scene_set_rigs before sthip_scene_upload");
  if (rig_count && !rigs) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, call + "rigs is NULL");
  std::vector<sthip_ctx::ResidentRig> next(rig_count);
  size_t records = 0, target_records = 0, bones = 0;
  for (uint32_t i = 0; i < rig_count; i++) {
    const sthip_rig_desc& d = rigs[i];
    const std::string rig = call + "rig " + std::to_string(i) + ": ";
    if ((uint64_t)d.first_vertex + d.vertex_count > ctx->vertex_count) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, rig + "the range ends past the vertex_count of the uploaded scene");
    if (d.blend_target_count > sthip::ANIMATE_MAX_TARGETS) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, rig + "blend_target_count is more than 4");
    if (d.bone_count > sthip::ANIMATE_MAX_BONES) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, rig + "bone_count is more than 1024");
    for (uint32_t t = 0; t < d.blend_target_count; t++)
      if (!d.blend_targets[t]) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, rig + "a blend target that blend_target_count requires is NULL");
    if (d.bone_count && !d.weights) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, rig + "bone_count > 0 but weights is NULL");
    for (uint32_t j = 0; j < i; j++)
      if (d.vertex_count && rigs[j].vertex_count && d.first_vertex < rigs[j].first_vertex + rigs[j].vertex_count && rigs[j].first_vertex < d.first_vertex + d.vertex_count)
        return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, rig + "its range overlaps the range of rig " + std::to_string(j));
    if (d.bone_count)
      for (uint32_t v = 0; v < d.vertex_count; v++)
        for (int k = 0; k < 4; k++)
          if (d.weights[v].indices[k] >= d.bone_count) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, rig + "a bone index of vertex " + std::to_string(v) + " is not below bone_count");
    sthip_ctx::ResidentRig& r = next[i];
    r.first = d.first_vertex;
    r.count = d.vertex_count;
    r.target_count = d.blend_target_count;
    r.bone_count = d.bone_count;
    r.at = records;
    r.targets_at = target_records;
    r.bones_at = bones;
    records += d.vertex_count;
    target_records += (size_t)d.blend_target_count * d.vertex_count;
    bones += d.bone_count;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ctx->scene_serial++;  // (first_hits.h)
  if (!rig_count) {
    drop_rigs(ctx);
    return STHIP_OK;
  }
  DevBuf<sthip_PackedVertexData> rest, targets;
  DevBuf<sthip_VertexWeight> weights;
  DevBuf<sthip_TransformData> bone_buf;
  HIP_TRY(ctx, rest.ensure(records));
  HIP_TRY(ctx, targets.ensure(target_records));
  HIP_TRY(ctx, weights.ensure(bones ? records : 0));  // (one place per rigged vertex, so that a rig's weights lie where its rest pose does)
  HIP_TRY(ctx, bone_buf.ensure(bones));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (an animate call before this one wrote the records the rest pose is taken from)
  for (uint32_t i = 0; i < rig_count; i++) {
    const sthip_ctx::ResidentRig& r = next[i];
    if (!r.count) continue;
    const size_t bytes = (size_t)r.count * sizeof(sthip_PackedVertexData);
    HIP_TRY(ctx, hipMemcpy(rest.p + r.at, ctx->vertices.p + r.first, bytes, hipMemcpyDeviceToDevice));
    for (uint32_t t = 0; t < r.target_count; t++) HIP_TRY(ctx, hipMemcpy(targets.p + r.targets_at + (size_t)t * r.count, rigs[i].blend_targets[t], bytes, hipMemcpyHostToDevice));
    if (r.bone_count) HIP_TRY(ctx, hipMemcpy(weights.p + r.at, rigs[i].weights, (size_t)r.count * sizeof(sthip_VertexWeight), hipMemcpyHostToDevice));
  }
  HIP_TRY(ctx, hipDeviceSynchronize());
  std::swap(ctx->rig_rest.p, rest.p), std::swap(ctx->rig_rest.n, rest.n);
  std::swap(ctx->rig_targets.p, targets.p), std::swap(ctx->rig_targets.n, targets.n);
  std::swap(ctx->rig_weights.p, weights.p), std::swap(ctx->rig_weights.n, weights.n);
  std::swap(ctx->rig_bones.p, bone_buf.p), std::swap(ctx->rig_bones.n, bone_buf.n);
  ctx->rigs.swap(next);
  ctx->rig_bones_host.assign(bones, sthip_TransformData{});
  ctx->rig_factors.assign(rig_count, std::array<float, 4>{{0, 0, 0, 0}});
  return STHIP_OK;
}

// sthip.h: the pose is checked and staged on the host; from there on the call is a vertex update whose records are written by
// k_animate instead of coming up from the host.
int sthip_scene_animate(sthip_ctx* ctx, const sthip_rig_pose* poses, uint32_t pose_count, sthip_refit_info* info) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  const auto t0 = std::chrono::steady_clock::now();
  if (info) memset(info, 0, sizeof(*info));
  const std::string call = "sthip_scene_animate: ";
  if (!ctx->has_scene) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_scene_animate before sthip_scene_upload");
  if (ctx->rigs.empty()) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_scene_animate before sthip_scene_set_rigs: no rigs are resident");
  if (pose_count != ctx->rigs.size()) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, call + "pose_count is not the rig_count of sthip_scene_set_rigs");
  if (!poses) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, call + "poses is NULL");
  for (uint32_t i = 0; i < pose_count; i++) {
    const sthip_ctx::ResidentRig& r = ctx->rigs[i];
    const std::string rig = call + "pose " + std::to_string(i) + ": ";
    for (uint32_t t = 0; t < r.target_count; t++)
      if (!std::isfinite(poses[i].blend_factors[t])) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, rig + "a blend factor is not finite");
    if (r.bone_count && !poses[i].bones) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, rig + "the rig has bones but bones is NULL");
    for (uint32_t b = 0; b < r.bone_count; b++)
      for (int e = 0; e < 12; e++)
        if (!std::isfinite(poses[i].bones[b].m[e / 4][e % 4])) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, rig + "an entry of bone " + std::to_string(b) + " is not finite");
  }
  for (uint32_t i = 0; i < pose_count; i++) {  // (nothing is staged from a call that is refused)
    const sthip_ctx::ResidentRig& r = ctx->rigs[i];
    for (uint32_t t = 0; t < 4; t++) ctx->rig_factors[i][t] = t < r.target_count ? poses[i].blend_factors[t] : 0.0f;
    if (r.bone_count) memcpy(ctx->rig_bones_host.data() + r.bones_at, poses[i].bones, (size_t)r.bone_count * sizeof(sthip_TransformData));
  }
  return update_resident_vertices(ctx, VertexSource{"sthip_scene_animate", nullptr, 0, 0}, info, t0);
}

int sthip_scene_read_image(sthip_ctx* ctx, uint32_t image_index, uint32_t level, void* out, uint64_t out_bytes) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  if (!ctx->has_scene) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_scene_read_image before sthip_scene_upload");
  if (image_index >= ctx->image_count || image_index >= ctx->images_host.size()) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_scene_read_image: image_index is not in gImages");
  const DeviceImage& im = ctx->images_host[image_index];
  if (level >= im.levels) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_scene_read_image: the image has " + std::to_string(im.levels) + " levels");
  const bool bytes = im.format == STHIP_IMAGE_FORMAT_RGBA8_UNORM;
  const uint64_t want = (uint64_t)im.w[level] * im.h[level] * (bytes ? 4u : 16u);
  if (!out || out_bytes != want) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_scene_read_image: the level holds " + std::to_string(want) + " bytes; out is NULL or out_bytes differs");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const void* src = bytes ? (const void*)(ctx->image_texels8.p + im.offset[level]) : (const void*)(ctx->image_texels.p + im.offset[level]);
  HIP_TRY(ctx, hipMemcpy(out, src, (size_t)want, hipMemcpyDeviceToHost));
  return STHIP_OK;
}

int sthip_scene_read_distributions(sthip_ctx* ctx, uint32_t first, uint32_t count, float* out) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  if (!ctx->has_scene) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_scene_read_distributions before sthip_scene_upload");
  if ((uint64_t)first + count > ctx->distribution_count) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_scene_read_distributions: the range ends past the distribution_count of the uploaded scene");
  if (!count) return STHIP_OK;
  if (!out) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_scene_read_distributions: out is NULL");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipMemcpy(out, ctx->distributions.p + first, (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
  return STHIP_OK;
}

// sthip.h. check (scene_prepare.cpp: nothing resident is touched before it has passed) -> reserve -> wait -> value, texels,
// mip chain, tables on the stream -> the kept scene follows
int sthip_scene_set_environment(sthip_ctx* ctx, const sthip_environment_desc* d, sthip_environment_info* info) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  const auto t0 = std::chrono::steady_clock::now();
  sthip::ResidentEnvironmentScene resident;
  resident.has_scene = ctx->has_scene;
  resident.materials = ctx->materials_host.data();
  resident.material_bytes = ctx->materials_host.size();
  resident.images = ctx->images_host.data();
  resident.image_count = (uint32_t)std::min<size_t>(ctx->image_count, ctx->images_host.size());
  resident.image_in_material = ctx->image_in_material.size() >= resident.image_count ? ctx->image_in_material.data() : nullptr;
  resident.distribution_count = ctx->distribution_count;
  sthip::EnvironmentPlan plan;
  int rc = STHIP_OK;
  std::string why;
  if (!sthip::check_environment(resident, d, plan, rc, why)) return fail(ctx, rc, why);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // everything that can run out of memory, before anything resident changes
  std::vector<double> sines;
  if (plan.build_tables) {
    sthip::environment_row_sines(plan.height, sines);
    HIP_TRY(ctx, ctx->env_sines.ensure(plan.height));
    HIP_TRY(ctx, ctx->env_integrals.ensure(plan.height));
  }
  if ((rc = make_edit_events(ctx)) != STHIP_OK) return rc;
  // frames in flight still read the old environment (sthip_render_async: their copies too, so that their tickets are complete)
  if ((rc = quiesce(ctx)) != STHIP_OK) return rc;
  ctx->reuse_grids_valid = false;  // (stored samples carry radiance of the environment they were taken in)
  hipStream_t st = ctx->stream;
  enum Stage { STAGE_BEGIN, STAGE_COPY, STAGE_MIPS, STAGE_SINES, STAGE_ROWS, STAGE_MARGINAL, STAGE_NORMALISE, STAGE_COUNT };
  StageTimer stages(environment_times_file(), plan.build_tables, STAGE_COUNT);
  HIP_TRY(ctx, hipEventRecord(ctx->edit_ev[0], st));
  stages.mark(STAGE_BEGIN, st);
  if (plan.set_value && (rc = write_material_bytes(ctx, d->material_address, d->value, 12, st)) != STHIP_OK) return rc;
  std::string err;
  if (plan.replace_pixels) {
    // (no record names the image now, but one may have and may again: a range kept from the old texels is forgotten, so that
    // sthip_scene_set_material_data scans the new ones when a record binds the image)
    if (plan.image_index < ctx->image_ranges.size()) ctx->image_ranges[plan.image_index] = sthip::ImageRange();
    // (the general path of sthip_scene_set_images: the format is the resident image's, which check_environment found to be RGBA32F)
    if ((rc = copy_image_level0(ctx, false, plan.image_index, d->pixels, d->device_ptr != 0, st)) != STHIP_OK) return rc;
    stages.mark(STAGE_COPY, st);
    if ((rc = rebuild_image_mips(ctx, plan.image_index, st, "sthip_scene_set_environment")) != STHIP_OK) return rc;
    stages.mark(STAGE_MIPS, st);
    kept_image_follows(ctx, false, plan.image_index, d->pixels, d->device_ptr != 0);
  }
  if (plan.build_tables) {
    const DeviceImage& im = ctx->images_host[plan.image_index];
    HIP_TRY(ctx, hipMemcpyAsync(ctx->env_sines.p, sines.data(), sines.size() * sizeof(double), hipMemcpyHostToDevice, st));
    sthip::EnvironmentTables t;
    t.texels = ctx->image_texels.p + im.offset[0];
    t.width = plan.width;
    t.height = plan.height;
    t.sines = ctx->env_sines.p;
    t.integrals = ctx->env_integrals.p;
    t.marginal_pdf = ctx->distributions.p + plan.table[0];
    t.row_pdf = ctx->distributions.p + plan.table[1];
    t.marginal_cdf = ctx->distributions.p + plan.table[2];
    t.row_cdf = ctx->distributions.p + plan.table[3];
    if (!plan.replace_pixels) {
      stages.mark(STAGE_COPY, st);
      stages.mark(STAGE_MIPS, st);
    }
    stages.mark(STAGE_SINES, st);
    bool ok = sthip::env_rows_launch(t, ctx->env_rows_per_wave, st, err);
    stages.mark(STAGE_ROWS, st);
    ok = ok && sthip::env_marginal_launch(t, st, err);
    stages.mark(STAGE_MARGINAL, st);
    ok = ok && sthip::env_normalise_launch(t, st, err);
    stages.mark(STAGE_NORMALISE, st);
    if (!ok) return fail(ctx, STHIP_ERR_HIP, "sthip_scene_set_environment: " + err);
    if (ctx->kept.valid && ctx->kept.distributions.size() == ctx->distribution_count) ctx->kept.stale_env_tables = true;
  }
  HIP_TRY(ctx, hipEventRecord(ctx->edit_ev[1], st));
  HIP_TRY(ctx, hipStreamSynchronize(st));  // (`sines` and a pageable `pixels` array are the caller's again from here on)
  static const char* const stage_names[STAGE_COUNT - 1] = {"copy_ms", "mips_ms", "sines_ms", "k_env_rows_ms", "k_env_marginal_ms", "k_env_normalise_ms"};
  stages.write("\"rows_per_wave\": " + std::to_string(ctx->env_rows_per_wave), stage_names);
  if (info) fill_edit_times(ctx, info, t0);
  return STHIP_OK;
}

// ---- sthip_scene_set_images / sthip_scene_set_material_data / sthip_scene_read_image_range (sthip.h) ----
// Room for the scan of `count` images by at most `blocks` blocks each: everything of it that can run out of memory
static int reserve_image_ranges(sthip_ctx* ctx, size_t count, uint32_t blocks) {
  if (!count) return STHIP_OK;
  HIP_TRY(ctx, ctx->range_partials.ensure((size_t)blocks * sthip::IMAGE_RANGE_PARTIAL_WORDS));
  HIP_TRY(ctx, ctx->range_results.ensure(count * sthip::IMAGE_RANGE_RESULT_WORDS));
  return STHIP_OK;
}
static uint32_t image_range_blocks_for(const sthip_ctx* ctx, const DeviceImage& im) {
  return sthip::image_range_blocks((uint64_t)im.w[0] * im.h[0], im.format == STHIP_IMAGE_FORMAT_RGBA8_UNORM, ctx->cu_count, ctx->image_range_blocks);
}
// k_image_range over level 0 of the images `scan` names, as they are resident in stream order; the partials are one buffer
// (the launches of one stream run one after the other), the results one 12-word record per image
static int enqueue_image_ranges(sthip_ctx* ctx, const std::vector<uint32_t>& scan, hipStream_t st, const char* call) {
  std::string err;
  for (size_t k = 0; k < scan.size(); k++) {
    const DeviceImage& im = ctx->images_host[scan[k]];
    const bool rgba8 = im.format == STHIP_IMAGE_FORMAT_RGBA8_UNORM;
    const void* src = rgba8 ? (const void*)(ctx->image_texels8.p + im.offset[0]) : (const void*)(ctx->image_texels.p + im.offset[0]);
    if (!sthip::image_range_launch(src, (uint64_t)im.w[0] * im.h[0], rgba8, image_range_blocks_for(ctx, im), ctx->range_partials.p, ctx->range_results.p + k * sthip::IMAGE_RANGE_RESULT_WORDS, st, err))
      return fail(ctx, STHIP_ERR_HIP, std::string(call) + ": " + err);
  }
  return STHIP_OK;
}
// The one read-back of a call (it waits for the stream), into the ranges the context keeps
static int fetch_image_ranges(sthip_ctx* ctx, const std::vector<uint32_t>& scan, hipStream_t st) {
  std::vector<uint32_t> words(scan.size() * sthip::IMAGE_RANGE_RESULT_WORDS);
  if (!scan.empty()) HIP_TRY(ctx, hipMemcpyAsync(words.data(), ctx->range_results.p, words.size() * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  for (size_t k = 0; k < scan.size(); k++) {
    sthip::ImageRange& r = ctx->image_ranges[scan[k]];
    const uint32_t* w = words.data() + k * sthip::IMAGE_RANGE_RESULT_WORDS;
    memcpy(r.lo, w, 16);
    memcpy(r.hi, w + 4, 16);
    r.nan_mask = w[8];
    r.known = 1;
  }
  return STHIP_OK;
}
// STHIP_MATERIAL_TIMES=<file> (StageTimer): every call that scans appends one line with the HIP-event time of its
// k_image_range launches alone
static const char* material_times_file() {
  static const char* const path = times_file("STHIP_MATERIAL_TIMES");
  return path;
}
static void write_range_times(StageTimer& times, const char* call, size_t images, uint32_t blocks) {
  static const char* const names[1] = {"k_image_range_ms"};
  times.write("\"call\": \"" + std::string(call) + "\", \"images\": " + std::to_string(images) + ", \"blocks\": " + std::to_string(blocks), names);
}
static sthip::MaterialAnalysis analyse_resident_materials(const sthip_ctx* ctx) {
  return sthip::analyse_materials(ctx->material_instances.data(), (uint32_t)ctx->material_instances.size(), ctx->materials_host.data(), (uint32_t)ctx->image_ranges.size(), ctx->image_ranges.data());
}
static void fill_images_info(sthip_ctx* ctx, sthip_images_info* info, bool before, size_t scanned, std::chrono::steady_clock::time_point t0) {
  if (!info) return;
  fill_edit_times(ctx, info, t0);
  info->has_specular_before = before ? 1u : 0u;
  info->has_specular_after = ctx->has_specular ? 1u : 0u;
  info->images_scanned = (uint32_t)scanned;
  info->pad = 0;
}

// check (scene_prepare.cpp) -> reserve -> wait -> texels, mip chains, scans on the stream -> one read-back -> the analysis again
// -> the kept scene follows
int sthip_scene_set_images(sthip_ctx* ctx, const sthip_image_update* entries, uint32_t n, uint32_t struct_size, sthip_images_info* info) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  const auto t0 = std::chrono::steady_clock::now();
  sthip::ResidentImages resident;
  resident.has_scene = ctx->has_scene;
  resident.images = ctx->images_host.data();
  resident.image_count = (uint32_t)std::min<size_t>(ctx->image_count, ctx->images_host.size());
  resident.images1 = ctx->images1_host.data();
  resident.image1_count = (uint32_t)ctx->images1_host.size();
  int rc = STHIP_OK;
  std::string why;
  if (!sthip::check_images(resident, entries, n, struct_size, rc, why)) return fail(ctx, rc, why);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<uint32_t> scan;  // the replaced images a material record names
  uint32_t blocks = 1;
  bool mask_changed = false;
  for (uint32_t k = 0; k < n; k++) {
    const sthip_image_update& e = entries[k];
    if (e.which) {
      mask_changed = true;
    } else if (e.index < ctx->image_in_material.size() && ctx->image_in_material[e.index] && e.index < ctx->image_ranges.size()) {
      scan.push_back(e.index);
      blocks = std::max(blocks, image_range_blocks_for(ctx, ctx->images_host[e.index]));
    }
  }
  if ((rc = reserve_image_ranges(ctx, scan.size(), blocks)) != STHIP_OK) return rc;
  if ((rc = make_edit_events(ctx)) != STHIP_OK) return rc;
  if ((rc = quiesce(ctx)) != STHIP_OK) return rc;  // frames in flight still read the old texels
  ctx->reuse_grids_valid = false;         // (stored samples carry the old materials' radiance)
  if (mask_changed) ctx->scene_serial++;  // (first_hits.h: the alpha test decides first hits; images of gImages alone move none)
  // the range the context holds for a replaced image is the old texels': forgotten here, and made again below for the images
  // a record names. An image nobody names stays unscanned until a record binds it (sthip_scene_set_material_data scans it then).
  for (uint32_t k = 0; k < n; k++)
    if (!entries[k].which && entries[k].index < ctx->image_ranges.size()) ctx->image_ranges[entries[k].index] = sthip::ImageRange();
  hipStream_t st = ctx->stream;
  HIP_TRY(ctx, hipEventRecord(ctx->edit_ev[0], st));
  for (uint32_t k = 0; k < n; k++) {
    const sthip_image_update& e = entries[k];
    if ((rc = copy_image_level0(ctx, e.which != 0, e.index, e.pixels, e.device_ptr != 0, st)) != STHIP_OK) return rc;
    if (!e.which && (rc = rebuild_image_mips(ctx, e.index, st, "sthip_scene_set_images")) != STHIP_OK) return rc;
  }
  StageTimer times(material_times_file(), !scan.empty(), 2);
  times.mark(0, st);
  if ((rc = enqueue_image_ranges(ctx, scan, st, "sthip_scene_set_images")) != STHIP_OK) return rc;
  times.mark(1, st);
  HIP_TRY(ctx, hipEventRecord(ctx->edit_ev[1], st));
  if ((rc = fetch_image_ranges(ctx, scan, st)) != STHIP_OK) return rc;  // (a pageable `pixels` array is the caller's again from here on)
  write_range_times(times, "sthip_scene_set_images", scan.size(), blocks);
  const bool before = ctx->has_specular;
  if (!scan.empty()) ctx->has_specular = analyse_resident_materials(ctx).has_specular;  // (nothing else of the analysis depends on texels)
  for (uint32_t k = 0; k < n; k++) kept_image_follows(ctx, entries[k].which != 0, entries[k].index, entries[k].pixels, entries[k].device_ptr != 0);
  fill_images_info(ctx, info, before, scan.size(), t0);
  return STHIP_OK;
}

// check (scene_prepare.cpp) -> reserve -> wait -> the bytes, the scans of images the analysis newly reads -> the analysis again
int sthip_scene_set_material_data(sthip_ctx* ctx, uint32_t offset, const void* data, uint32_t bytes, sthip_images_info* info) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  const auto t0 = std::chrono::steady_clock::now();
  sthip::ResidentMaterials resident;
  resident.has_scene = ctx->has_scene;
  resident.materials = ctx->materials_host.data();
  resident.material_bytes = ctx->materials_host.size();
  resident.instances = ctx->material_instances.data();
  resident.instance_count = (uint32_t)ctx->material_instances.size();
  resident.image_count = (uint32_t)std::min<size_t>(ctx->image_count, ctx->images_host.size());
  resident.image1_count = (uint32_t)ctx->images1_host.size();
  resident.volume_count = ctx->volume_count;
  int rc = STHIP_OK;
  std::string why;
  std::vector<uint8_t> edited;
  if (!sthip::check_material_data(resident, offset, data, bytes, edited, rc, why)) return fail(ctx, rc, why);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // an image whose range the analysis reads now and nobody has scanned (a record names it for the first time, or under a
  // constant that has become positive): scanned from the resident texels
  std::vector<uint8_t> named, range_read;
  sthip::material_images(resident.instances, resident.instance_count, edited.data(), (uint32_t)ctx->image_ranges.size(), named, range_read);
  std::vector<uint32_t> scan;
  uint32_t blocks = 1;
  for (uint32_t i = 0; i < range_read.size() && i < resident.image_count; i++)
    if (range_read[i] && !ctx->image_ranges[i].known) {
      scan.push_back(i);
      blocks = std::max(blocks, image_range_blocks_for(ctx, ctx->images_host[i]));
    }
  if ((rc = reserve_image_ranges(ctx, scan.size(), blocks)) != STHIP_OK) return rc;
  if ((rc = make_edit_events(ctx)) != STHIP_OK) return rc;
  if ((rc = quiesce(ctx)) != STHIP_OK) return rc;  // frames in flight still read the old records
  ctx->reuse_grids_valid = false;  // (stored samples carry the old materials' radiance)
  hipStream_t st = ctx->stream;
  HIP_TRY(ctx, hipEventRecord(ctx->edit_ev[0], st));
  if (bytes && (rc = write_material_bytes(ctx, offset, data, bytes, st)) != STHIP_OK) return rc;
  StageTimer times(material_times_file(), !scan.empty(), 2);
  times.mark(0, st);
  if ((rc = enqueue_image_ranges(ctx, scan, st, "sthip_scene_set_material_data")) != STHIP_OK) return rc;
  times.mark(1, st);
  HIP_TRY(ctx, hipEventRecord(ctx->edit_ev[1], st));
  if ((rc = fetch_image_ranges(ctx, scan, st)) != STHIP_OK) return rc;
  write_range_times(times, "sthip_scene_set_material_data", scan.size(), blocks);
  const bool before = ctx->has_specular;
  sthip::MaterialAnalysis m = analyse_resident_materials(ctx);
  if (m.inst_flags.size() == ctx->inst_flags_host.size() && m.inst_flags != ctx->inst_flags_host)
    HIP_TRY(ctx, hipMemcpy(ctx->inst_flags.p, m.inst_flags.data(), m.inst_flags.size(), hipMemcpyHostToDevice));
  ctx->inst_flags_host = std::move(m.inst_flags);
  ctx->has_specular = m.has_specular;
  ctx->textured = m.textured;
  ctx->image_in_material = std::move(m.image_in_material);
  fill_images_info(ctx, info, before, scan.size(), t0);
  return STHIP_OK;
}

int sthip_scene_read_image_range(sthip_ctx* ctx, uint32_t image_index, float lo[4], float hi[4], uint32_t* nan_mask) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  if (!ctx->has_scene) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_scene_read_image_range before sthip_scene_upload");
  if (image_index >= ctx->image_count || image_index >= ctx->image_ranges.size()) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_scene_read_image_range: image_index is not in gImages");
  const sthip::ImageRange& r = ctx->image_ranges[image_index];
  if (!r.known || image_index >= ctx->image_in_material.size() || !ctx->image_in_material[image_index])
    return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_scene_read_image_range: the context holds no range for gImages[" + std::to_string(image_index) + "] (no material record names it under a constant with a positive component)");
  if (lo) memcpy(lo, r.lo, 16);
  if (hi) memcpy(hi, r.hi, 16);
  if (nan_mask) *nan_mask = r.nan_mask;
  return STHIP_OK;
}

int sthip_scene_read_vertices(sthip_ctx* ctx, uint32_t first_vertex, uint32_t vertex_count, sthip_PackedVertexData* out) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  if (!ctx->has_scene) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_scene_read_vertices before sthip_scene_upload");
  if ((uint64_t)first_vertex + vertex_count > ctx->vertex_count)
    return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_scene_read_vertices: the range ends past the vertex_count of the uploaded scene");
  if (!vertex_count) return STHIP_OK;
  if (!out) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_scene_read_vertices: out is NULL");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipMemcpy(out, ctx->vertices.p + first_vertex, (size_t)vertex_count * sizeof(sthip_PackedVertexData), hipMemcpyDeviceToHost));
  return STHIP_OK;
}

// One hash grid from one seed's staged appends (hashgrid.h): compact the stage in (path, vertex) order, hash the keys, build
// the table the serial probe sequence of find_or_insert would build (hashgrid.hlsli:43-58; in parallel: hashgrid.hip), prefix
// the bucket counters (compute_indices, :72-79) and scatter the records into their bucket ranges (swizzle, :81-88) — all of it
// enqueued on the stream, nothing visits the host. appends == nullptr (sthip_build_hash_grid's keys form): hg_keys / hg_count
// hold the keys already, and there are no records to compact or scatter.
static int build_hash_grid(sthip_ctx* ctx, hipStream_t st, const float4* appends, float4* compact, float4* data, size_t slots, uint32_t rec, uint32_t flag_at, bool lvc_records,
                           uint32_t bucket_count, DevBuf<uint32_t>& d_checksums, DevBuf<uint32_t>& d_counters, DevBuf<uint32_t>& d_indices) {
  const uint32_t buckets = bucket_count + 32u;  // probing does not wrap
  const unsigned kgrid = (unsigned)((slots + STHIP_BLOCK - 1) / STHIP_BLOCK);
  if (appends) {
    size_t tmp_bytes = ctx->hg_tmp.n;
    HIP_TRY(ctx, sthip::lvc_compact(appends, (uint32_t)slots, 1, (uint32_t)slots, compact, ctx->hg_count.p, ctx->hg_flags.p, ctx->hg_offsets.p, ctx->hg_tmp.p, tmp_bytes, st, rec, flag_at));
    if (lvc_records)
      hipLaunchKernelGGL(k_hg_keys_lvc, dim3(kgrid), dim3(STHIP_BLOCK), 0, st, compact, ctx->hg_count.p, bucket_count, ctx->hg_keys.p);
    else
      hipLaunchKernelGGL(k_hg_keys, dim3(kgrid), dim3(STHIP_BLOCK), 0, st, compact, ctx->hg_count.p, bucket_count, ctx->hg_keys.p);
  }
  // the probe sequence, the bucket ranges and every record's place, on the device (hashgrid.hip): no host hop
  size_t build_bytes = ctx->hg_tmp.n;
  HIP_TRY(ctx, sthip::hashgrid_build_device(ctx->hg_keys.p, ctx->hg_count.p, (uint32_t)slots, buckets, d_checksums.p, d_counters.p, d_indices.p, ctx->hg_dest.p, ctx->hg_owner.p, ctx->hg_bucket_of.p,
                                            ctx->hg_append.p, ctx->hg_sorted_bucket.p, ctx->hg_sorted_append.p, ctx->hg_key64.p, ctx->hg_sorted_key64.p, ctx->hg_tmp.p, build_bytes, st, ctx->hashgrid_serial));
  if (appends) {
    if (lvc_records)
      hipLaunchKernelGGL(k_hg_scatter_lvc, dim3(kgrid), dim3(STHIP_BLOCK), 0, st, compact, ctx->hg_count.p, ctx->hg_dest.p, data);
    else
      hipLaunchKernelGGL(k_hg_scatter, dim3(kgrid), dim3(STHIP_BLOCK), 0, st, compact, ctx->hg_count.p, ctx->hg_dest.p, data);
  }
  HIP_TRY(ctx, hipGetLastError());
  return STHIP_OK;
}

// The buffers of a reuse grid's build at `hg_slots` append slots and `hg_buckets` table slots (DevBuf::ensure keeps what is large
// enough): the stage, its compaction and the bucket ranges of the record kinds asked for, the table, hashgrid.hip's scratch, and
// the two temp-size queries. sthip_render's plan and sthip_build_hash_grid size them here.
static int reserve_hash_grid_buffers(sthip_ctx* ctx, size_t hg_slots, uint32_t hg_buckets, bool nee, bool lvc) {
  if (nee) {
    HIP_TRY(ctx, ctx->hg_appends.ensure(4 * hg_slots));
    HIP_TRY(ctx, ctx->hg_compact.ensure(4 * hg_slots));
    HIP_TRY(ctx, ctx->hg_data.ensure(3 * hg_slots));
  }
  if (lvc) {
    HIP_TRY(ctx, ctx->lg_appends.ensure(6 * hg_slots));
    HIP_TRY(ctx, ctx->lg_compact.ensure(6 * hg_slots));
    HIP_TRY(ctx, ctx->lg_data.ensure(5 * hg_slots));
    for (DevBuf<uint32_t>* b : {&ctx->lg_checksums, &ctx->lg_counters, &ctx->lg_indices}) HIP_TRY(ctx, b->ensure(hg_buckets));
  }
  for (DevBuf<uint32_t>* b : {&ctx->hg_flags, &ctx->hg_offsets, &ctx->hg_dest, &ctx->hg_bucket_of, &ctx->hg_append, &ctx->hg_sorted_bucket, &ctx->hg_sorted_append}) HIP_TRY(ctx, b->ensure(hg_slots));
  for (DevBuf<unsigned long long>* b : {&ctx->hg_key64, &ctx->hg_sorted_key64}) HIP_TRY(ctx, b->ensure(hg_slots));
  for (DevBuf<uint32_t>* b : {&ctx->hg_checksums, &ctx->hg_counters, &ctx->hg_indices}) HIP_TRY(ctx, b->ensure(hg_buckets));
  HIP_TRY(ctx, ctx->hg_keys.ensure(hg_slots));
  HIP_TRY(ctx, ctx->hg_count.ensure(1));
  HIP_TRY(ctx, ctx->hg_owner.ensure(hg_buckets + 2 + 1024));  // (+ hashgrid.hip's control words and special-cell list)
  size_t tmp_bytes = 0, build_bytes = 0;
  HIP_TRY(ctx, sthip::lvc_compact(nullptr, (uint32_t)hg_slots, 1, 0, nullptr, nullptr, ctx->hg_flags.p, ctx->hg_offsets.p, nullptr, tmp_bytes, ctx->stream));
  HIP_TRY(ctx, sthip::hashgrid_build_device(nullptr, nullptr, (uint32_t)hg_slots, hg_buckets, nullptr, ctx->hg_counters.p, ctx->hg_indices.p, nullptr, nullptr, ctx->hg_bucket_of.p, ctx->hg_append.p,
                                            ctx->hg_sorted_bucket.p, ctx->hg_sorted_append.p, ctx->hg_key64.p, ctx->hg_sorted_key64.p, nullptr, build_bytes, ctx->stream));
  HIP_TRY(ctx, ctx->hg_tmp.ensure(std::max<size_t>(16, std::max(tmp_bytes, build_bytes))));
  return STHIP_OK;
}

// The reuse grid's build on its own (include/sthip.h): the keys, or staged records, of the caller through build_hash_grid on the
// buffers a render builds in, and everything it left copied back. The grids kept for the next render are dropped.
int sthip_build_hash_grid(sthip_ctx* ctx, const sthip_hash_grid_desc* d, sthip_hash_grid_info* info) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  auto refuse = [&](const char* field, const std::string& why) { return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, std::string("sthip_build_hash_grid: ") + field + " " + why); };
  if (!d) return refuse("desc", "is NULL");
  if (!info) return refuse("info", "is NULL");
  if (d->struct_size != sizeof(sthip_hash_grid_desc)) return refuse("struct_size", "is not sizeof(sthip_hash_grid_desc)");
  if (d->form > 2u) return refuse("form", "is not 0 (keys), 1 (NEE records) or 2 (LVC records)");
  if (d->bucket_count == 0 || d->bucket_count > (1u << 28)) return refuse("bucket_count", "is outside (0, 2^28]");
  if (d->slots == 0 || d->slots > 0x7FFFFFFFu) return refuse("slots", "is outside [1, 2^31 - 1]");
  const bool records = d->form != 0, lvc = d->form == 2;
  if (!records && d->count > d->slots) return refuse("count", "is above slots");
  if (!d->checksums) return refuse("checksums", "is NULL");
  if (!d->counters) return refuse("counters", "is NULL");
  if (!d->indices) return refuse("indices", "is NULL");
  if (!d->dest) return refuse("dest", "is NULL");
  if (records) {
    if (!d->records) return refuse("records", "is NULL");
    if (!d->compacted_keys) return refuse("compacted_keys", "is NULL");
    if (!d->data) return refuse("data", "is NULL");
  } else {
    if (d->count && !d->keys) return refuse("keys", "is NULL");
    for (uint32_t k = 0; k < d->count; k++) {
      if (d->keys[2 * (size_t)k] >= d->bucket_count) return refuse("keys", "[" + std::to_string(k) + "]: the home bucket is not below bucket_count");
      if (d->keys[2 * (size_t)k + 1] == 0u) return refuse("keys", "[" + std::to_string(k) + "]: a checksum of 0 marks an empty slot");
    }
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ctx->reuse_grids_valid = false;  // (the table and the records of the last render are overwritten)
  const size_t slots = d->slots;
  const uint32_t buckets = d->bucket_count + 32u, rec = lvc ? 6u : 4u, out_rec = lvc ? 5u : 3u;
  const int rc = reserve_hash_grid_buffers(ctx, slots, buckets, d->form == 1, lvc);
  if (rc != STHIP_OK) return rc;
  hipStream_t st = ctx->stream;
  DevBuf<uint32_t>&d_checksums = lvc ? ctx->lg_checksums : ctx->hg_checksums, &d_counters = lvc ? ctx->lg_counters : ctx->hg_counters, &d_indices = lvc ? ctx->lg_indices : ctx->hg_indices;
  float4 *appends = nullptr, *compact = nullptr, *data = nullptr;
  if (records) {
    appends = lvc ? ctx->lg_appends.p : ctx->hg_appends.p;
    compact = lvc ? ctx->lg_compact.p : ctx->hg_compact.p;
    data = lvc ? ctx->lg_data.p : ctx->hg_data.p;
    HIP_TRY(ctx, hipMemcpyAsync(appends, d->records, slots * rec * sizeof(float4), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(data, 0, slots * out_rec * sizeof(float4), st));  // (a render reads the records the build placed only)
  } else {
    if (d->count) HIP_TRY(ctx, hipMemcpyAsync(ctx->hg_keys.p, d->keys, (size_t)d->count * sizeof(uint2), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->hg_count.p, &d->count, sizeof(uint32_t), hipMemcpyHostToDevice, st));
  }
  HIP_TRY(ctx, hipStreamSynchronize(st));  // (the sources are the caller's pageable memory)
  const int rc2 = build_hash_grid(ctx, st, appends, compact, data, slots, rec, lvc ? 0u : 2u, lvc, d->bucket_count, d_checksums, d_counters, d_indices);
  if (rc2 != STHIP_OK) return rc2;
  uint32_t count = 0, ctl[2] = {0, 0};
  HIP_TRY(ctx, hipMemcpyAsync(&count, ctx->hg_count.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(ctl, ctx->hg_owner.p + buckets, sizeof ctl, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(d->checksums, d_checksums.p, buckets * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(d->counters, d_counters.p, buckets * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(d->indices, d_indices.p, buckets * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (count > slots) return fail(ctx, STHIP_ERR_HIP, "sthip_build_hash_grid: the device counted more appends than slots");
  if (count) HIP_TRY(ctx, hipMemcpyAsync(d->dest, ctx->hg_dest.p, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (records) {
    if (count) HIP_TRY(ctx, hipMemcpyAsync(d->compacted_keys, ctx->hg_keys.p, (size_t)count * sizeof(uint2), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(d->data, data, slots * out_rec * sizeof(float4), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(ctx, hipStreamSynchronize(st));
  info->count = count;
  info->special_cells = ctl[1];
  info->serial_rebuild = ctl[0];
  info->dropped = 0;
  for (uint32_t k = 0; k < count; k++) info->dropped += d->dest[k] == 0xFFFFFFFFu ? 1u : 0u;
  return STHIP_OK;
}

// The buffers sthip_render sizes by the number of paths in flight (released before a second attempt with half the batch)
static void release_path_state(sthip_ctx* ctx) {
  (void)hipStreamSynchronize(ctx->stream);  // an earlier call's kernels may still read them
  ctx->ray_o.release();
  ctx->ray_d.release();
  ctx->hit.release();
  ctx->beta.release();
  ctx->radiance.release();
  ctx->shadow_sum.release();
  ctx->shadow_rays.release();
  ctx->light_vertices.release();
  ctx->conn.release();
  ctx->media_state.release();
  ctx->shade_stack.release();
  ctx->shadow_hit.release();
  ctx->shadow_ext.release();
  ctx->shadow_result.release();
  ctx->cone.release();
  ctx->meta.release();
  ctx->queue0.release();
  ctx->queue1.release();
  ctx->queue_kept.release();
  ctx->bdpt.release();
  ctx->rr.release();
  ctx->cs_nee.release();
  ctx->cs_lvc.release();
  ctx->lvc_staging.release();
  ctx->lvc_flags.release();
  ctx->lvc_offsets.release();
  ctx->lvc_tmp.release();
  ctx->path_contrib.release();
  ctx->light_trace.release();
  ctx->presampled.release();
  ctx->deep_rays.release();
  // the kept first hits are a cache: the device is short of memory, so they go too (the next attempt traces the first bounce)
  ctx->first_hit.release();
  ctx->first_hit_leaf.release();
  ctx->first_hits_valid = false;
}

// ---- the render call: plan_render, reserve_render_buffers, bind_frame_params, run_batches, read_back ----

static uint32_t owned_tiles(uint32_t tiles, uint32_t shard_rank, uint32_t shard_count) { return tiles > shard_rank ? (tiles - shard_rank + shard_count - 1) / shard_count : 0; }

// What a render call resolves from its arguments and the context before it touches the device (plan_render): the resolved
// flags and push constants, which techniques run, the sizes of the path state, the round counts, the kernels. Plain data that
// the later phases read.
struct RenderPlan {
  sthip_BDPTPushConstants pc;
  uint32_t sampling_flags, scene_flags, view_count, debug_mode;
  bool has_env, media, inline_media, nee, connect_views, connect_paths, bdpt, light_tracing, lvc, lvc_reservoirs, nee_reuse, lvc_reuse;
  bool coherent_rr, coherent_nee, coherent_lvc, presample, ext, shadow_debug, dev, out_packed, every_entry_written;
  uint32_t W, H, tiles_x, tiles_y, paths_per_seed, path_count, batch, hg_buckets, light_threads, primary_rays, grid, lds_material_bytes;
  uint32_t max_bounce_rounds, drain_rounds, max_shadow_round;
  size_t pixels, P, P0, seg_stride, shadow_stride, shadow_entries, hg_slots, lvc_slots, vertices_per_seed, conn_per_path, radiance_entries, presample_n;
  uint64_t reuse_key[3];
  const void *k_trace[2], *k_shade, *k_probe, *k_shade_light;  // k_trace without / with traversal counters; the view pass's k_shade and its probe
  uint32_t shade_lds, probe_lds;
  // "reuse_first_hits": the call's first bounce may be served from / kept in the context's buffers, and what for (first_hits.h).
  // plan_render says whether the call is of that kind; reserve_render_buffers withdraws it if the buffers cannot be had.
  bool keep_first_hits;
  sthip::FirstHitKey first_hit_key;
};

// primary rays = owned pixels that lie inside the image and inside a view (known without asking the GPU)
static uint32_t count_primary_rays(const RenderPlan& r, const sthip_ctx* ctx, const sthip_frame_desc* frame) {
  uint32_t primary_rays = 0;
  if (r.pc.gMaxPathVertices < 2) return 0;
  for (uint32_t t = ctx->shard_rank; t < r.tiles_x * r.tiles_y; t += ctx->shard_count) {
    const uint32_t ty = t / r.tiles_x, tx = t - ty * r.tiles_x;
    const int x0 = (int)(tx * ctx->tile_w), y0 = (int)(ty * ctx->tile_h);
    const int x1 = (int)std::min(r.W, (tx + 1) * ctx->tile_w), y1 = (int)std::min(r.H, (ty + 1) * ctx->tile_h);
    if (r.view_count == 1) {
      const int ax0 = std::max(x0, frame->gViews[0].image_min[0]), ay0 = std::max(y0, frame->gViews[0].image_min[1]);
      const int ax1 = std::min(x1, frame->gViews[0].image_max[0]), ay1 = std::min(y1, frame->gViews[0].image_max[1]);
      if (ax1 > ax0 && ay1 > ay0) primary_rays += (uint32_t)(ax1 - ax0) * (uint32_t)(ay1 - ay0);
    } else {
      for (int y = y0; y < y1; y++)
        for (int x = x0; x < x1; x++)
          for (uint32_t v = 0; v < r.view_count; v++) {
            const sthip_ViewData& vw = frame->gViews[v];
            if (x >= vw.image_min[0] && y >= vw.image_min[1] && x < vw.image_max[0] && y < vw.image_max[1]) {
              primary_rays++;
              break;
            }
          }
    }
  }
  return primary_rays;
}

// Flag resolution and every argument check of a render call. No HIP call, no allocation, and the context is only read (but for
// ctx->error and, once the plan is valid, the two stats the out-of-memory retry goes by): a rejected call leaves it as it was.
static int plan_render(sthip_ctx* ctx, const sthip_BDPTPushConstants* pc_in, uint32_t sampling_flags, uint32_t scene_flags, const sthip_frame_desc* frame, uint32_t seed_count, const sthip_outputs* out,
                       RenderPlan& r) {
  if (!pc_in || !frame || !out || !out->gRadiance || !frame->gViews || !frame->gViewTransforms || frame->view_count == 0 || seed_count == 0)
    return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: a required argument is NULL/zero");
  if (!ctx->has_scene) return fail(ctx, STHIP_ERR_NO_SCENE, "no scene uploaded");
  if (pc_in->gViewCount != frame->view_count) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: gViewCount != frame.view_count");
  if ((out->gDepth || out->gPrevUVs) && !frame->gInverseViewTransforms && !frame->gPrevInverseViewTransforms)
    return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: depth / prev-uv outputs need gInverseViewTransforms");
  // BDPT_FLAG_TRACE_LIGHT is a per-kernel specialisation of the reference (sample_photons), never a caller's choice
  if (scene_flags & STHIP_BDPT_FLAG_TRACE_LIGHT) return fail(ctx, STHIP_ERR_UNSUPPORTED, "render: BDPT_FLAG_TRACE_LIGHT is not a scene flag a caller sets");
  const uint32_t unsupported = (1u << STHIP_eSampleLightPower);
  if (sampling_flags & unsupported) return fail(ctx, STHIP_ERR_UNSUPPORTED, "render: a sampling flag outside the built hot path is set");
  if (pc_in->gMaxPathVertices > 60 || pc_in->gMaxDiffuseVertices > 60) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: path length limits above 60");
  if (pc_in->gLightCount > ctx->light_count) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: gLightCount exceeds the uploaded light list");

  // flag resolution of BDPT::render (BDPT.cpp:486-523), idempotent if the host has done it already
  memset(&r, 0, sizeof(r));
  sthip_BDPTPushConstants& pcn = r.pc;
  pcn = *pc_in;
  if (pcn.gLightCount == 0) scene_flags &= ~STHIP_BDPT_FLAG_HAS_EMISSIVES;
  const bool has_env = (scene_flags & STHIP_BDPT_FLAG_HAS_ENVIRONMENT) != 0, has_emissives = (scene_flags & STHIP_BDPT_FLAG_HAS_EMISSIVES) != 0;
  if (!has_env) pcn.gEnvironmentSampleProbability = 0;
  if (!has_emissives) pcn.gEnvironmentSampleProbability = 1;
  if (!has_emissives && !has_env) sampling_flags &= ~((1u << STHIP_eNEE) | (1u << STHIP_eConnectToViews) | (1u << STHIP_eConnectToLightPaths));
  if (!(sampling_flags & (1u << STHIP_eNEE))) sampling_flags &= ~((1u << STHIP_ePresampleLights) | (1u << STHIP_eNEEReservoirs) | (1u << STHIP_eNEEReservoirReuse));
  if (!(sampling_flags & (1u << STHIP_eNEEReservoirs))) sampling_flags &= ~(1u << STHIP_eNEEReservoirReuse);  // only connect_light_reservoir touches the grid
  if (!(sampling_flags & (1u << STHIP_eLVC))) sampling_flags &= ~((1u << STHIP_eLVCReservoirs) | (1u << STHIP_eLVCReservoirReuse));  // BDPT.cpp:517-520
  if (!(sampling_flags & (1u << STHIP_eConnectToLightPaths))) sampling_flags &= ~((1u << STHIP_eLVC) | (1u << STHIP_eLVCReservoirs) | (1u << STHIP_eLVCReservoirReuse));  // only connect_lvc reads the cache
  if (!(sampling_flags & (1u << STHIP_eLVCReservoirs))) sampling_flags &= ~(1u << STHIP_eLVCReservoirReuse);  // the reuse sits inside connect_lvc's reservoir branch
  if (!(sampling_flags & ((1u << STHIP_eNEE) | (1u << STHIP_eLVC)))) sampling_flags &= ~(1u << STHIP_eDeferShadowRays);  // BDPT.cpp:522-523
  // eCoherentSampling only touches the index of a presampled light (path.hlsli:317,379) and connect_lvc's (:688,703)
  if (!(sampling_flags & ((1u << STHIP_ePresampleLights) | (1u << STHIP_eLVC)))) sampling_flags &= ~(1u << STHIP_eCoherentSampling);
  const sthip_BDPTPushConstants* pc = &pcn;
  r.sampling_flags = sampling_flags;
  r.scene_flags = scene_flags;
  r.has_env = has_env;
  r.view_count = frame->view_count;
  const auto flag = [&](uint32_t bit) { return (sampling_flags & (1u << bit)) != 0; };
  if (has_env) {  // the Environment record (environment.h:17-22): ImageValue3, then 4 offsets into gDistributions when an image is bound
    const size_t addr = pcn.gEnvironmentMaterialAddress;
    if (addr + 16 > ctx->materials_host.size() || (addr & 3)) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: gEnvironmentMaterialAddress is outside gMaterialData");
    uint32_t rec[8] = {0};
    memcpy(rec, ctx->materials_host.data() + addr, 16);
    if (rec[3] < STHIP_IMAGE_COUNT) {
      if (rec[3] >= ctx->image_count || addr + 32 > ctx->materials_host.size()) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: the environment refers to an image that is not in gImages");
      // (the environment's lookups and its texel descent read the float array at every level: shading.h, Environment)
      if (rec[3] < ctx->images_host.size() && ctx->images_host[rec[3]].format != STHIP_IMAGE_FORMAT_RGBA32F)
        return fail(ctx, STHIP_ERR_UNSUPPORTED, "render: the environment map is an 8-bit image (gImages[" + std::to_string(rec[3]) + "] is RGBA8_UNORM): upload it as RGBA32F");
      memcpy(rec, ctx->materials_host.data() + addr, 32);
      const size_t w = ctx->image_dims[rec[3]].first, h = ctx->image_dims[rec[3]].second;
      const size_t need[4] = {h, w * h, h + 1, (w + 1) * h};  // marginal_pdf, row_pdf, marginal_cdf, row_cdf (dist2.h)
      for (int k = 0; k < 4; k++)
        if ((size_t)rec[4 + k] + need[k] > ctx->distribution_count) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: an environment distribution table lies outside gDistributions");
    }
  }

  // participating media (BDPT_FLAG_HAS_MEDIA, BDPT.cpp:497-500)
  if (ctx->has_volumes && !(scene_flags & STHIP_BDPT_FLAG_HAS_MEDIA)) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: the scene has volume instances but BDPT_FLAG_HAS_MEDIA is not set");
  const bool media = r.media = ctx->has_volumes;
  if (media && flag(STHIP_eCoherentSampling)) return fail(ctx, STHIP_ERR_UNSUPPORTED, "render: eCoherentSampling with media (walks through volumes break the lockstep of a workgroup)");
  // With media every visibility ray draws random numbers. A deferred NEE ray carries its own offset (k_shadow_media walks it);
  // everything else draws from the path's own stream in the middle of a vertex — NEE without eDeferShadowRays, light tracing's
  // connect_view, the connections to stored light vertices or to the light vertex cache — and k_shade / k_shade_light walk those
  // themselves (visibility_walk_media).
  if (!media) pcn.gMaxNullCollisions = 0;
  const uint32_t W = r.W = pc->gOutputExtent[0], H = r.H = pc->gOutputExtent[1];
  if (W == 0 || H == 0) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: empty output extent");
  r.pixels = (size_t)W * H;
  r.tiles_x = (W + ctx->tile_w - 1) / ctx->tile_w;
  r.tiles_y = (H + ctx->tile_h - 1) / ctx->tile_h;
  r.paths_per_seed = owned_tiles(r.tiles_x * r.tiles_y, ctx->shard_rank, ctx->shard_count) * ctx->tile_w * ctx->tile_h;
  // Seeds traced together in one pass. A shard of a frame is small (1/8 of 1080p = 259 K paths does not fill
  // 256 CUs of persistent waves), so several seeds of the owned pixels share the launches, up to ~4 M paths.
  const uint32_t max_in_flight = (uint32_t)std::max<uint64_t>(1, (ctx->max_paths_in_flight) / std::max(1u, r.paths_per_seed));
  // Reservoir reuse couples the seeds of a call: seed s looks into the hash grid seed s - 1 built (the reference's frame
  // and previous frame), so they are traced one at a time and the grid is built between them.
  const bool nee_reuse = r.nee_reuse = flag(STHIP_eNEEReservoirReuse);
  const bool lvc_reuse = r.lvc_reuse = flag(STHIP_eLVCReservoirReuse);
  // BDPTDebugMode: upstream's gDebugImage persists from frame to frame and most modes add to it or overwrite it: the seeds of a
  // call are traced one after the other, as its frames are
  const uint32_t debug_mode = r.debug_mode = out->gDebugImage ? out->debug_mode : 0u;
  if (debug_mode >= STHIP_DEBUG_MODE_COUNT) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: debug_mode is not a BDPTDebugMode");
  const uint32_t batch = r.batch = (nee_reuse || lvc_reuse || debug_mode) ? 1u : std::min(seed_count, max_in_flight);
  r.path_count = batch * r.paths_per_seed;
  // light tracing (eConnectToViews, BDPT.cpp:653-667): sample_photons' padded dispatch, dispatch_over(W, ceil(gLightPathCount / W))
  const bool connect_views = r.connect_views = flag(STHIP_eConnectToViews);
  const bool connect_paths = r.connect_paths = flag(STHIP_eConnectToLightPaths);  // light-subpath connections, no light vertex cache
  const bool bdpt = r.bdpt = connect_views || connect_paths;
  const bool light_tracing = r.light_tracing = bdpt && pc->gMaxPathVertices > 2;
  if (bdpt) {
    if (has_env) return fail(ctx, STHIP_ERR_UNSUPPORTED, "render: light subpaths with an environment (upstream starts environment light paths from an unset position, bdpt.hlsl:109-113)");
    if (!frame->gInverseViewTransforms) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: eConnectToViews / eConnectToLightPaths need gInverseViewTransforms");
    if (connect_paths && !flag(STHIP_eRemapThreads) && (W & 7u))
      return fail(ctx, STHIP_ERR_UNSUPPORTED, "render: eConnectToLightPaths without eRemapThreads needs a width that is a multiple of 8 (upstream's padding threads race on the vertex slots of the next row)");
    if (connect_paths && pc->gMaxDiffuseVertices < 1) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: eConnectToLightPaths needs gMaxDiffuseVertices >= 1");
  }
  const bool lvc = r.lvc = connect_paths && flag(STHIP_eLVC);
  r.lvc_reservoirs = lvc && flag(STHIP_eLVCReservoirs);
  if (lvc) {
    if (pc->gMaxDiffuseVertices < 2) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: eLVC needs gMaxDiffuseVertices >= 2 (a light path stores vertices 1 .. gMaxDiffuseVertices - 1)");
    if (pc->gLightPathCount == 0 || (uint64_t)pc->gLightPathCount * pc->gMaxDiffuseVertices > (1ull << 28)) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: eLVC needs 0 < gLightPathCount * gMaxDiffuseVertices <= 2^28");
  }
  const uint32_t light_rows = (pc->gLightPathCount + W - 1) / W;
  const uint32_t light_threads = r.light_threads = light_tracing ? ((W + 7) / 8) * 8 * ((light_rows + 3) / 4) * 4 : 0;
  if ((uint64_t)light_threads * batch > 0x7FFFFFFFull || (light_tracing && (uint64_t)batch * W * H > 0x7FFFFFFFull)) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: too many light paths in flight");
  const size_t P = r.P = std::max<size_t>(std::max<size_t>(1, r.path_count), (size_t)light_threads * batch);
  r.P0 = std::max<size_t>(1, r.paths_per_seed);
  r.vertices_per_seed = connect_paths ? (size_t)pc->gLightPathCount * pc->gMaxDiffuseVertices : 0;
  const size_t conn_per_path = r.conn_per_path = connect_paths ? pc->gMaxDiffuseVertices - 1 : 0;
  if (connect_paths && (uint64_t)P * std::max<size_t>(1, conn_per_path) >= 0x40000000ull) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: too many connection entries in flight");
  if (lvc) {
    r.lvc_slots = (size_t)pc->gLightPathCount * (pc->gMaxDiffuseVertices - 1) * batch;
    if (r.lvc_slots > 0x7FFFFFFFull) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: too many light-vertex-cache slots in flight");
  }

  r.hg_buckets = (nee_reuse || lvc_reuse) ? pc->gHashGridBucketCount + 32u : 0u;  // probing does not wrap (hashgrid.h)
  if (nee_reuse || lvc_reuse) {
    if (has_env) return fail(ctx, STHIP_ERR_UNSUPPORTED, "render: eNEEReservoirReuse with an environment (a stored environment sample is read back as a surface point upstream: sample_Le leaves its pdfA positive)");
    if (ctx->shard_count > 1) return fail(ctx, STHIP_ERR_UNSUPPORTED, "render: eNEEReservoirReuse on a pixel-tile shard (the grid is a whole-frame structure: render replicas and reduce)");
    if (pc->gHashGridBucketCount == 0 || pc->gHashGridBucketCount > (1u << 28) || !(pc->gHashGridMinBucketRadius > 0)) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: eNEEReservoirReuse needs 0 < gHashGridBucketCount <= 2^28 and gHashGridMinBucketRadius > 0");
    r.hg_slots = (size_t)((W + 7) / 8) * ((H + 3) / 4) * 32 * std::max(1u, pc->gMaxDiffuseVertices);  // covers both map_pixel_coord forms
    if (r.hg_slots > 0x7FFFFFFFull) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: too many hash-grid append slots");
  }
  // what the grids of this call are built for: the first seed looks into the ones the previous call left only if the key is the same
  r.reuse_key[0] = (uint64_t)(nee_reuse ? 1u : 0u) | (lvc_reuse ? 2u : 0u);
  r.reuse_key[1] = r.hg_buckets;
  r.reuse_key[2] = r.hg_slots;

  // The queues are cut into QUEUE_SEGMENTS segments (traverse.h). A segment starts as a contiguous eighth of the
  // slots and only shrinks from bounce to bounce, which bounds it and the distance between segments.
  r.grid = std::max<uint32_t>(grid_for(ctx, P), QUEUE_SEGMENTS);
  r.seg_stride = (((P + QUEUE_SEGMENTS - 1) / QUEUE_SEGMENTS) + 63) & ~(size_t)63;
  if (r.seg_stride * QUEUE_SEGMENTS > 0xFFFFFFFFull) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: too many paths in flight");
  // a vertex queues at most one NEE ray, plus one visibility ray per stored light vertex it connects to
  // (media: the walks of earlier vertices are still in the queue when a vertex adds its own — at most one per diffuse vertex and path)
  r.shadow_stride = r.seg_stride * (media ? std::max<size_t>(1, pc->gMaxDiffuseVertices) : 1 + conn_per_path);
  if (r.shadow_stride * QUEUE_SEGMENTS > 0xFFFFFFFFull) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: too many shadow rays in flight");
  r.shadow_entries = r.shadow_stride * QUEUE_SEGMENTS;  // per round; media ping-pong between two such regions
  if (media && 2 * r.shadow_entries > 0xFFFFFFFFull) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: too many shadow rays in flight");
  // ePresampleLights (BDPT.cpp:644-651): gLightPresampleTileSize x TileCount light points per seed in flight
  r.presample = flag(STHIP_ePresampleLights) && pc->gMaxPathVertices > 2;
  r.presample_n = (size_t)pc->gLightPresampleTileSize * pc->gLightPresampleTileCount;
  if (flag(STHIP_ePresampleLights)) {
    if (has_env) return fail(ctx, STHIP_ERR_UNSUPPORTED, "render: ePresampleLights with an environment (upstream leaves the presampled environment direction unset, bdpt.hlsl:93)");
    if (r.presample_n == 0 || r.presample_n > (1u << 24)) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: gLightPresampleTileSize * gLightPresampleTileCount must be in 1 .. 2^24");
  }
  if (media && frame->gViewMediumInstances)
    for (uint32_t v = 0; v < frame->view_count; v++) {
      const uint32_t mi = frame->gViewMediumInstances[v];
      if (mi != 0xFFFFu && (mi >= ctx->instance_count || !ctx->instance_is_volume[mi])) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: gViewMediumInstances entry is not a volume instance");
    }
  if (out->radiance_layout > STHIP_LAYOUT_SHARD_TILES) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render: unknown radiance_layout");

  // eCoherentRR takes effect in rounds in which a path can reach the roulette (shade_view_round); never with media
  r.coherent_rr = flag(STHIP_eCoherentRR) && !media;
  // eCoherentSampling: one probe per site and round (FrameParams::cs_nee / cs_lvc)
  r.coherent_nee = flag(STHIP_eCoherentSampling) && flag(STHIP_ePresampleLights) && flag(STHIP_eNEE);
  r.coherent_lvc = flag(STHIP_eCoherentSampling) && lvc;
  r.nee = flag(STHIP_eNEE);
  r.inline_media = media && r.nee && !flag(STHIP_eDeferShadowRays);
  if (debug_mode) {
    // inline shadow rays add to the debug image only where they are unoccluded: they are traced once more, with what they add
    const bool inline_adds = (debug_mode == STHIP_DEBUG_RESERVOIR_WEIGHT || (debug_mode == STHIP_DEBUG_PATH_LENGTH_CONTRIBUTION && pc->gDebugLightPathLength == 1)) && r.nee &&
                             !flag(STHIP_eDeferShadowRays) && !media;
    // so do light-subpath connections (accumulate_contribution with the light vertex's length, path.hlsli:797,820); connect_lvc's
    // deferred record (:781-789) adds to the radiance only
    const bool connection_adds = debug_mode == STHIP_DEBUG_PATH_LENGTH_CONTRIBUTION && pc->gDebugLightPathLength >= 2 && connect_paths && !media && !(flag(STHIP_eLVC) && flag(STHIP_eDeferShadowRays));
    r.shadow_debug = inline_adds || connection_adds;
  }
  r.dev = out->device_ptrs != 0;
  r.out_packed = out->radiance_layout == STHIP_LAYOUT_SHARD_TILES;
  r.radiance_entries = r.out_packed ? std::max<size_t>(1, r.paths_per_seed) : r.pixels;
  r.primary_rays = count_primary_rays(r, ctx, frame);
  // Pixels this shard does not own and pixels outside every view are zero (a sum-reduce over shards assembles the frame).
  // When the shard is the whole frame and every pixel lies in a view, every output entry is written by the pass itself —
  // the first vertex's G-buffer stores (hit or miss) and k_resolve — so the five fills (131 MB at 1080p) are left out.
  r.every_entry_written = ctx->shard_count == 1 && !r.out_packed && !media && pc->gMaxPathVertices >= 2 && (size_t)r.primary_rays == r.pixels;
  // closest-hit rays per path <= gMaxPathVertices - 1 (path.hlsli:960); without specular materials every scattering
  // vertex counts as a diffuse vertex, so the path also ends after gMaxDiffuseVertices + 1 rays (path.hlsli:964-966):
  // rounds beyond that would only be empty launches
  r.max_bounce_rounds = pc->gMaxPathVertices >= 2 ? pc->gMaxPathVertices - 1 : 0;
  if (!ctx->has_specular) r.max_bounce_rounds = std::min(r.max_bounce_rounds, pc->gMaxDiffuseVertices + 1);
  // media: a trace() call walks from volume boundary to volume boundary, one k_trace round per segment (up to 2 per
  // volume instance and ray); a shadow ray likewise, so its last segments need rounds of their own after the last bounce.
  // The queue control words exist for 64 rounds; paths / shadow rays still walking after that are dropped.
  if (media) {
    r.drain_rounds = std::min(8u, 2 * ctx->volume_instances + 1);
    r.max_bounce_rounds = std::min<uint64_t>(62 - r.drain_rounds, (uint64_t)r.max_bounce_rounds * (1 + 2 * ctx->volume_instances));
  }
  // The deepest round whose vertices can queue a visibility ray. Without specular materials the vertex shaded in round d is
  // diffuse vertex d + 1, and the diffuse budget ends a path before NEE (path.hlsli:964-966 precede :978): rounds beyond
  // gMaxDiffuseVertices - 1 leave their shadow queue empty, and the launch that would trace it is left out.
  r.max_shadow_round = 0xFFFFFFFFu;
  if (!ctx->has_specular && !media && !bdpt) r.max_shadow_round = pc->gMaxDiffuseVertices ? pc->gMaxDiffuseVertices - 1 : 0u;

  // the kernels (kernel_variants.h): a variant that was never instantiated is an error of this call, not something to compile here
  r.ext = ctx->has_spheres || has_env || bdpt || flag(STHIP_eNEEReservoirs) || flag(STHIP_eShadingNormalShadowFix);
  r.lds_material_bytes = (ctx->lds_materials && !ctx->textured && ctx->materials_host.size() <= 32768) ? (uint32_t)(ctx->materials_host.size() & ~(size_t)3) : 0u;
  const int media_mode = media ? (r.inline_media ? 2 : 1) : 0;
  const bool alpha = (ctx->has_alpha && flag(STHIP_eAlphaTest)) || ctx->has_volumes;  // alpha masks under eAlphaTest, volume instances: the instantiation that carries them
  char tuple[96];
  const auto missing = [&]() { return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, std::string("render: no instantiation ") + tuple + " in kernel_variants.h"); };
  for (int probe = 0; probe < 2; probe++) {
    if (probe && !(r.coherent_rr || r.coherent_nee || r.coherent_lvc)) break;
    const sthip::ShadeVariant v = sthip::select_shade_variant(ctx->textured, r.ext, bdpt, media_mode, probe != 0, debug_mode != 0);
    snprintf(tuple, sizeof tuple, "k_shade<%d, %d, %d, %d, %d, %d>", v.textured, v.ext, v.lt, v.media, v.probe, v.debug);
    if (!((probe ? r.k_probe : r.k_shade) = find_kernel(g_shade_kernels, sthip::shade_key(v.textured, v.ext, v.lt, v.media, v.probe, v.debug)))) return missing();
    (probe ? r.probe_lds : r.shade_lds) = sthip::shade_lds_bytes(v, r.lds_material_bytes);
  }
  for (int count = 0; count < 2; count++) {
    r.k_trace[count] = trace_kernel(ctx->bvh, count != 0, alpha, ctx->bvh.top_count != 0);
    snprintf(tuple, sizeof tuple, "k_trace<%d, %d, %d, %d> of the resident tree", count, alpha, ctx->bvh.spill != nullptr, ctx->bvh.top_count != 0);
    if (!r.k_trace[count]) return missing();
  }
  if (light_tracing) {
    r.k_shade_light = find_kernel(g_shade_light_kernels, sthip::shade_light_key(ctx->textured, true, media));
    snprintf(tuple, sizeof tuple, "k_shade_light<%d, 1, %d>", ctx->textured, media);
    if (!r.k_shade_light) return missing();
  }
  // The first bounce from kept hits: only where run_batches traces it with the packet kernel (no volumes, a path budget of two
  // vertices or more, no debug mode that returns before tracing), and never under the diagnostic options, whose passes
  // describe the kernels (ms_trace_primary, nodes_visited_primary, rays_primary_packets of a traced first bounce)
  r.keep_first_hits = ctx->reuse_first_hits && ctx->packet_primary && !ctx->has_volumes && !ctx->count_traversal && !ctx->time_kernels && r.max_bounce_rounds >= 1 && r.paths_per_seed > 0 &&
                      debug_mode != STHIP_DEBUG_ENVIRONMENT_SAMPLE_TEST && debug_mode != STHIP_DEBUG_ENVIRONMENT_SAMPLE_PDF &&
                      sthip::first_hit_key_make(r.first_hit_key, ctx->scene_serial, pc->gOutputExtent, r.view_count, pc->gMaxPathVertices, ctx->shard_rank, ctx->shard_count, ctx->tile_w, ctx->tile_h,
                                                r.paths_per_seed, ctx->has_alpha && flag(STHIP_eAlphaTest), flag(STHIP_eFlipTriangleUVs), frame->gViews, frame->gViewTransforms);
  ctx->stats.leaf_records = (!ctx->bvh.wide8_nodes && ctx->bvh.wide_nodes && ctx->bvh.pairs && !alpha) ? 1u : 0u;  // (trace_kernel's rule)
  ctx->stats.paths_per_seed = r.paths_per_seed;
  ctx->stats.seeds_in_flight = batch;
  return STHIP_OK;
}

// Every buffer the call needs, at the sizes of the plan (DevBuf::ensure keeps what is large enough), and the two temp-size queries
static int reserve_render_buffers(sthip_ctx* ctx, RenderPlan& r, const sthip_outputs* out, AsyncSlot* slot) {
  const size_t P = r.P, hg_slots = r.hg_slots, shadow_entries = r.shadow_entries, queue_entries = r.seg_stride * QUEUE_SEGMENTS;
  if (r.bdpt) {
    HIP_TRY(ctx, ctx->bdpt.ensure(P));
    if (r.light_tracing && r.connect_views) HIP_TRY(ctx, ctx->light_trace.ensure((size_t)r.batch * r.W * r.H * 4));
    if (r.connect_paths) {
      HIP_TRY(ctx, ctx->light_vertices.ensure(4 * std::max<size_t>(1, r.vertices_per_seed * r.batch)));
      HIP_TRY(ctx, ctx->conn.ensure(std::max<size_t>(1, (size_t)r.path_count * r.conn_per_path)));
    }
    if (r.lvc) {
      HIP_TRY(ctx, ctx->lvc_staging.ensure(4 * r.lvc_slots));
      HIP_TRY(ctx, ctx->lvc_flags.ensure(r.lvc_slots));
      HIP_TRY(ctx, ctx->lvc_offsets.ensure(r.lvc_slots));
      HIP_TRY(ctx, ctx->lvc_count.ensure(r.batch));
      size_t tmp_bytes = 0;
      HIP_TRY(ctx, sthip::lvc_compact(nullptr, (uint32_t)(r.lvc_slots / r.batch), r.batch, 0, nullptr, nullptr, ctx->lvc_flags.p, ctx->lvc_offsets.p, nullptr, tmp_bytes, ctx->stream));
      HIP_TRY(ctx, ctx->lvc_tmp.ensure(std::max<size_t>(16, tmp_bytes)));
      if (r.lvc_reservoirs) HIP_TRY(ctx, ctx->path_contrib.ensure(P));
    }
  }
  if (r.nee_reuse || r.lvc_reuse) {
    const int rc = reserve_hash_grid_buffers(ctx, hg_slots, r.hg_buckets, r.nee_reuse, r.lvc_reuse);
    if (rc != STHIP_OK) return rc;
  }

  for (DevBuf<float4>* b : {&ctx->ray_o, &ctx->ray_d, &ctx->hit, &ctx->beta, &ctx->radiance, &ctx->shadow_sum}) HIP_TRY(ctx, b->ensure(P));
  HIP_TRY(ctx, ctx->hit_leaf.ensure(P));
  HIP_TRY(ctx, ctx->accum.ensure(r.P0));
  if (ctx->textured || r.debug_mode) HIP_TRY(ctx, ctx->cone.ensure(P));  // (a debug mode runs the general instantiation of k_shade)
  if (r.debug_mode) HIP_TRY(ctx, ctx->debug.ensure(P));
  HIP_TRY(ctx, ctx->shadow_rays.ensure(3 * shadow_entries * (r.media ? 2 : 1)));
  if (ctx->bvh.spill) {  // bounded LDS stacks: room for every ray of a trace launch to overflow (4 x float4 each)
    HIP_TRY(ctx, ctx->deep_rays.ensure(4 * (P + shadow_entries)));
    if (ctx->deep_count.n < 2) {  // [0] rays in the deep queue, [1] k_trace_deep blocks that are through: both zero between launches (k_trace_deep resets them)
      HIP_TRY(ctx, ctx->deep_count.ensure(2));
      HIP_TRY(ctx, hipMemsetAsync(ctx->deep_count.p, 0, 8, ctx->stream));
    }
  }
  if (r.media) {
    HIP_TRY(ctx, ctx->media_state.ensure(2 * P));
    HIP_TRY(ctx, ctx->shadow_hit.ensure(2 * shadow_entries));
    HIP_TRY(ctx, ctx->shadow_ext.ensure(2 * shadow_entries));
    HIP_TRY(ctx, ctx->shadow_result.ensure(P * std::max(1u, r.pc.gMaxDiffuseVertices)));
    HIP_TRY(ctx, ctx->view_medium.ensure(std::max(1u, r.view_count)));
  }
  HIP_TRY(ctx, ctx->meta.ensure(P));
  for (DevBuf<uint32_t>* b : {&ctx->queue0, &ctx->queue1, &ctx->queue_kept}) HIP_TRY(ctx, b->ensure(queue_entries));
  HIP_TRY(ctx, ctx->counters.ensure(CNT_TOTAL));
  HIP_TRY(ctx, ctx->qctl.ensure((size_t)3 * 64 * QUEUE_SEGMENTS * QCTL_STRIDE));  // path queues, shadow queues, and (BDPTDebugMode) the shadow rays' debug halves
  if (r.sampling_flags & (1u << STHIP_ePresampleLights)) HIP_TRY(ctx, ctx->presampled.ensure(2 * r.presample_n * r.batch));
  const size_t vbytes = (size_t)r.view_count * 48, params_bytes = 5 * vbytes + (size_t)r.view_count * 4;
  HIP_TRY(ctx, ctx->views.ensure(5 * vbytes));
  if (slot && slot->params_cap < params_bytes) {  // the pipelined form keeps the call's arrays in the slot's pinned block
    if (slot->params) (void)hipHostFree(slot->params);
    slot->params = nullptr;
    slot->params_cap = 0;
    HIP_TRY(ctx, hipHostMalloc((void**)&slot->params, params_bytes, hipHostMallocDefault));
    slot->params_cap = params_bytes;
  }
  if (r.coherent_rr) HIP_TRY(ctx, ctx->rr.ensure(P));
  if (r.coherent_nee) HIP_TRY(ctx, ctx->cs_nee.ensure(P));
  if (r.coherent_lvc) HIP_TRY(ctx, ctx->cs_lvc.ensure(P));
  if (r.inline_media || (r.media && r.bdpt))  // (light tracing's connect_view and the light-subpath connections walk inline whatever eDeferShadowRays says)
    HIP_TRY(ctx, ctx->shade_stack.ensure((size_t)r.grid * STHIP_BLOCK * std::max(1u, ctx->bvh.stack_depth)));

  // outputs: device pointers are written in place, host pointers go through staging buffers
  const size_t cb = ctx->color_bytes(), pixels = r.pixels;  // bytes of one colour-image entry (radiance, albedo, debug)
  const auto color_entries = [](size_t n, size_t bytes) { return (n * bytes + 15) / 16; };  // float4 entries of a staging buffer
  if (r.debug_mode && !r.dev) HIP_TRY(ctx, ctx->out_debug.ensure(color_entries(pixels, cb)));
  if (r.shadow_debug) HIP_TRY(ctx, ctx->shadow_debug.ensure(ctx->shadow_rays.n));
  if (!r.dev) {
    // the synchronous form has one staging set per context; a frame of sthip_render_async has its slot's, which the copy
    // stream reads while the next frame renders into another (allocated at first use, released when the frame's size changes)
    if (slot && (slot->key[0] != pixels || slot->key[1] != r.radiance_entries || slot->key[2] != cb)) {
      slot->release_images();
      slot->key[0] = pixels;
      slot->key[1] = r.radiance_entries;
      slot->key[2] = cb;
    }
    HIP_TRY(ctx, (slot ? slot->radiance : ctx->out_radiance).ensure(color_entries(r.radiance_entries, cb)));
    if (out->gAlbedo) HIP_TRY(ctx, (slot ? slot->albedo : ctx->out_albedo).ensure(color_entries(pixels, cb)));
    if (out->gVisibility) HIP_TRY(ctx, (slot ? slot->visibility : ctx->out_visibility).ensure(pixels));
    if (out->gDepth) HIP_TRY(ctx, (slot ? slot->depth : ctx->out_depth).ensure(pixels));
    if (out->gPrevUVs) HIP_TRY(ctx, (slot ? slot->prev_uv : ctx->out_prev_uv).ensure(pixels));
    if (slot) HIP_TRY(ctx, slot->counters.ensure(CNT_TOTAL));
  }
  // half colour precision: k_shade writes the albedo in binary32 to a stage, k_resolve rounds it into the caller's image (or its staging)
  if (ctx->half_color && out->gAlbedo) HIP_TRY(ctx, ctx->albedo_stage.ensure(pixels));
  // Last, when everything the call cannot do without is there: the kept first hits of one seed's paths. A device that cannot
  // hold them renders as without the option: no error, and nothing for the out-of-memory retry to halve a batch over.
  if (r.keep_first_hits && (ctx->first_hit.n < r.paths_per_seed || ctx->first_hit_leaf.n < r.paths_per_seed)) {
    ctx->first_hits_valid = false;  // (the buffers they are in go away)
    hipError_t e = ctx->first_hit.ensure(r.paths_per_seed);
    if (e == hipSuccess) e = ctx->first_hit_leaf.ensure(r.paths_per_seed);
    // (the leaf of an all-dead packet's slot is never written by the packet kernel and never used: only read, behind `ip != miss`)
    if (e == hipSuccess) e = hipMemsetAsync(ctx->first_hit_leaf.p, 0xFF, (size_t)r.paths_per_seed * sizeof(uint32_t), ctx->stream);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      ctx->first_hit.release();
      ctx->first_hit_leaf.release();
      r.keep_first_hits = false;
    }
  }
  return STHIP_OK;
}

// Fills the kernels' parameter block from the plan and the reserved buffers, uploads the view arrays, and clears what of the
// outputs the pass will not write itself. The first phase that enqueues work.
static int bind_frame_params(sthip_ctx* ctx, const RenderPlan& r, const sthip_frame_desc* frame, const sthip_outputs* out, AsyncSlot* slot, FrameParams& p) {
  hipStream_t st = ctx->stream;
  const size_t pixels = r.pixels, cb = ctx->color_bytes(), vbytes = (size_t)r.view_count * 48;
  memset(&p, 0, sizeof(p));
  p.pc = r.pc;
  p.sampling_flags = r.sampling_flags;
  p.scene_flags = r.scene_flags;
  p.shard_rank = ctx->shard_rank;
  p.shard_count = ctx->shard_count;
  p.tile_w = ctx->tile_w;
  p.tile_h = ctx->tile_h;
  p.tiles_x = r.tiles_x;
  p.tiles_y = r.tiles_y;
  p.paths_per_seed = r.paths_per_seed;
  p.path_count = r.path_count;
  {
    std::vector<uint8_t> stack_copy(slot ? 0 : 5 * vbytes);
    uint8_t* const host = slot ? slot->params : stack_copy.data();
    const void* const arrays[5] = {frame->gViews, frame->gViewTransforms, frame->gPrevViews ? (const void*)frame->gPrevViews : frame->gViews,
                                   frame->gPrevInverseViewTransforms ? frame->gPrevInverseViewTransforms : frame->gInverseViewTransforms, frame->gInverseViewTransforms};
    for (int k = 0; k < 5; k++)  // (an array the caller left out is zero)
      arrays[k] ? memcpy(host + k * vbytes, arrays[k], vbytes) : memset(host + k * vbytes, 0, vbytes);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->views.p, host, 5 * vbytes, hipMemcpyHostToDevice, st));
    if (!slot) HIP_TRY(ctx, hipStreamSynchronize(st));  // `stack_copy` goes out of scope (the slot's block lives until the slot's next frame, which waits for this one)
  }
  p.views = reinterpret_cast<const sthip_ViewData*>(ctx->views.p);
  p.view_xf = reinterpret_cast<const sthip_TransformData*>(ctx->views.p + vbytes);
  p.prev_views = reinterpret_cast<const sthip_ViewData*>(ctx->views.p + 2 * vbytes);
  p.prev_inv_view_xf = reinterpret_cast<const sthip_TransformData*>(ctx->views.p + 3 * vbytes);
  p.inv_view_xf = reinterpret_cast<const sthip_TransformData*>(ctx->views.p + 4 * vbytes);
  p.bdpt = r.bdpt ? ctx->bdpt.p : nullptr;
  p.light_trace = r.light_tracing && r.connect_views ? ctx->light_trace.p : nullptr;
  p.light_trace_empty = r.connect_views && !r.light_tracing ? 1u : 0u;
  p.light_vertices = r.connect_paths ? ctx->light_vertices.p : nullptr;
  p.conn = r.connect_paths && r.conn_per_path ? ctx->conn.p : nullptr;
  p.lds_material_bytes = r.lds_material_bytes;
  p.hg_checksums = ctx->hg_checksums.p;
  p.hg_counters = ctx->hg_counters.p;
  p.hg_indices = ctx->hg_indices.p;
  p.hg_data = ctx->hg_data.p;
  // the first seed of the call looks into the grids the previous call left, if it left them for the same estimator and table
  p.hg_prev = ((r.nee_reuse || r.lvc_reuse) && ctx->reuse_persist && ctx->reuse_grids_valid && !memcmp(r.reuse_key, ctx->reuse_key, sizeof r.reuse_key)) ? 1u : 0u;
  if (r.nee_reuse || r.lvc_reuse) ctx->reuse_grids_valid = false;  // (until this call has left its own)
  p.hg_appends = r.nee_reuse ? ctx->hg_appends.p : nullptr;
  p.lg_checksums = ctx->lg_checksums.p;
  p.lg_counters = ctx->lg_counters.p;
  p.lg_indices = ctx->lg_indices.p;
  p.lg_data = ctx->lg_data.p;
  p.lg_appends = r.lvc_reuse ? ctx->lg_appends.p : nullptr;
  p.lvc_staging = r.lvc ? ctx->lvc_staging.p : nullptr;
  p.lvc_count = r.lvc ? ctx->lvc_count.p : nullptr;
  p.path_contrib = r.lvc_reservoirs ? ctx->path_contrib.p : nullptr;
  p.light_threads = r.light_threads;
  p.light_trace_quantization = 65536;  // BDPT.hpp:55 mLightTraceQuantization

  p.bvh = ctx->bvh;
  p.bvh.alpha_test = (ctx->has_alpha && (r.sampling_flags & (1u << STHIP_eAlphaTest))) ? 1u : 0u;  // intersection.hlsli:118
  p.bvh.flip_uvs = (r.sampling_flags & (1u << STHIP_eFlipTriangleUVs)) ? 1u : 0u;
  p.scene.vertices = ctx->vertices.p;
  p.scene.indices = ctx->indices.p;
  p.scene.instances = ctx->instances.p;
  p.scene.xf = ctx->xf.p;
  p.scene.inv_xf = ctx->inv_xf.p;
  p.scene.motion_xf = ctx->motion_xf.p;
  p.scene.materials = ctx->materials.p;
  p.scene.lights = ctx->lights.p;
  p.scene.instance_count = ctx->instance_count;
  p.scene.light_count = ctx->light_count;
  p.scene.images = ctx->images.p;
  p.scene.image_texels = ctx->image_texels.p;
  p.scene.image_texels8 = ctx->image_texels8.p;
  p.scene.image_count = ctx->image_count;
  p.scene.distributions = ctx->distributions.p;
  p.scene.distribution_count = ctx->distribution_count;
  p.scene.volume_words = ctx->volume_words.p;
  p.scene.volumes = ctx->volumes.p;
  p.scene.volume_count = ctx->volume_count;
  p.scene.leaf_tris = ctx->bvh.tris;
  p.scene.leaf_shade = reinterpret_cast<const float4*>(ctx->tri_shade.p);
  p.ray_o = ctx->ray_o.p;
  p.ray_d = ctx->ray_d.p;
  p.hit = ctx->hit.p;
  p.hit_leaf = ctx->hit_leaf.p;
  p.beta = ctx->beta.p;
  p.meta = ctx->meta.p;
  p.radiance = ctx->radiance.p;
  p.shadow_sum = ctx->shadow_sum.p;
  p.accum = ctx->accum.p;
  p.cone = (ctx->textured || r.debug_mode) ? ctx->cone.p : nullptr;
  p.queue[0] = ctx->queue0.p;
  p.queue[1] = ctx->queue1.p;
  p.shadow_rays = ctx->shadow_rays.p;
  p.deep_rays = ctx->deep_rays.p;
  p.deep_count = ctx->deep_count.p;
  p.presampled = ctx->presampled.p;
  p.counters = ctx->counters.p;
  p.qctl = ctx->qctl.p;
  p.seg_stride = (uint32_t)r.seg_stride;
  p.shadow_stride = (uint32_t)r.shadow_stride;
  p.media = r.media ? 1u : 0u;
  p.inline_media = r.inline_media ? 1u : 0u;
  if (r.inline_media || (r.media && r.bdpt)) p.shade_stack = ctx->shade_stack.p;
  if (r.media) {
    p.shadow_alt = (uint32_t)r.shadow_entries;
    p.media_state = ctx->media_state.p;
    p.shadow_hit = ctx->shadow_hit.p;
    p.shadow_ext = ctx->shadow_ext.p;
    p.shadow_result = ctx->shadow_result.p;
    if (frame->gViewMediumInstances) {
      if (slot) {  // (the caller's array is borrowed for the call only: the upload reads the slot's pinned copy)
        memcpy(slot->params + 5 * vbytes, frame->gViewMediumInstances, (size_t)r.view_count * 4);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->view_medium.p, slot->params + 5 * vbytes, (size_t)r.view_count * 4, hipMemcpyHostToDevice, st));
      } else {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->view_medium.p, frame->gViewMediumInstances, (size_t)r.view_count * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
      }
      p.view_medium = ctx->view_medium.p;
    }
  }
  p.count_traversal = ctx->count_traversal ? 1u : 0u;
  p.refill_idle = ctx->refill_idle;
  p.inst_flags = ctx->inst_flags.p;
  p.emitters = ctx->emitters.p;
  p.emitter_count = 0;  // (set where the view pass starts: only the plain pipeline answers last rays)
  p.no_specular = ctx->has_specular ? 0u : 1u;
  p.inner_min_lanes = ctx->inner_min_lanes;
  p.rounds = r.max_bounce_rounds + r.drain_rounds;

  p.out_half = ctx->half_color ? 1u : 0u;
  p.debug_mode = r.debug_mode;
  p.debug = r.debug_mode ? ctx->debug.p : nullptr;
  if (r.debug_mode) {
    if (r.dev) {
      p.out_debug = out->gDebugImage;
    } else {  // in / out: what the caller's image holds goes up first
      HIP_TRY(ctx, hipMemcpyAsync(ctx->out_debug.p, out->gDebugImage, pixels * cb, hipMemcpyHostToDevice, st));
      p.out_debug = ctx->out_debug.p;
    }
    if (r.shadow_debug) p.shadow_debug = ctx->shadow_debug.p;
  }
  p.out_packed = r.out_packed ? 1u : 0u;
  if (r.dev) {
    p.out_radiance = out->gRadiance;
    p.out_albedo = reinterpret_cast<float4*>(out->gAlbedo);
    p.out_visibility = out->gVisibility;
    p.out_depth = out->gDepth;
    p.out_prev_uv = reinterpret_cast<float2*>(out->gPrevUVs);
  } else {
    p.out_radiance = slot ? slot->radiance.p : ctx->out_radiance.p;
    if (out->gAlbedo) p.out_albedo = slot ? slot->albedo.p : ctx->out_albedo.p;
    if (out->gVisibility) p.out_visibility = slot ? slot->visibility.p : ctx->out_visibility.p;
    if (out->gDepth) p.out_depth = slot ? slot->depth.p : ctx->out_depth.p;
    if (out->gPrevUVs) p.out_prev_uv = slot ? slot->prev_uv.p : ctx->out_prev_uv.p;
  }
  if (ctx->half_color && p.out_albedo) {
    p.out_albedo16 = reinterpret_cast<Half4*>(p.out_albedo);
    p.out_albedo = ctx->albedo_stage.p;
  }
  // The next writer of a staging set — the fills below or the first G-buffer store — runs after the copy of the frame that used
  // the set before (a no-op for an event that was never recorded). The binary32 albedo stage of half colour precision is one
  // per context: only k_shade and k_resolve touch it, in stream order; the copy reads the slot's RGBA16F image.
  if (slot) HIP_TRY(ctx, hipStreamWaitEvent(st, slot->copied, 0));
  if (!r.every_entry_written) {
    HIP_TRY(ctx, hipMemsetAsync(p.out_radiance, 0, r.radiance_entries * cb, st));
    if (p.out_albedo) HIP_TRY(ctx, hipMemsetAsync(p.out_albedo, 0, pixels * 16, st));
    if (p.out_albedo16) HIP_TRY(ctx, hipMemsetAsync(p.out_albedo16, 0, pixels * 8, st));
    if (p.out_visibility) HIP_TRY(ctx, hipMemsetAsync(p.out_visibility, 0, pixels * 8, st));
    if (p.out_depth) HIP_TRY(ctx, hipMemsetAsync(p.out_depth, 0, pixels * 16, st));
    if (p.out_prev_uv) HIP_TRY(ctx, hipMemsetAsync(p.out_prev_uv, 0, pixels * 8, st));
  }
  return STHIP_OK;
}

// What the launches of one render call share
struct RenderRun {
  sthip_ctx* ctx;
  const RenderPlan& plan;
  hipStream_t st;
  uint32_t tgrid;  // blocks of a k_trace launch (persistent: what is resident at once)
  size_t lds;      // ... and its dynamic LDS
};

// One k_trace launch over the path queue of round `dc` and the shadow queue of round `ds` (TRACE_NONE: none) and, for a tree
// higher than the LDS stack (the bounded instantiation), k_trace_deep for the rays that overflowed
static void launch_trace(const RenderRun& run, const FrameParams& p, uint32_t dc, uint32_t ds, bool count) {
  launch_kernel(run.plan.k_trace[count ? 1 : 0], run.tgrid, run.lds, run.st, p, dc, ds);
  if (p.bvh.spill) {
    const bool alpha = p.bvh.alpha_test || run.ctx->has_volumes;
    launch_kernel(STHIP_KERNEL2(k_trace_deep, count, alpha), (uint32_t)run.ctx->cu_count * 8u, 0, run.st, p);  // one spill column per thread (configure_stack)
  }
}

// The view pass's shading of round `depth`: the probes of eCoherentRR / eCoherentSampling, then the round's k_shade
static void shade_view_round(const RenderRun& run, FrameParams& p, uint32_t depth) {
  sthip_ctx* ctx = run.ctx;
  const RenderPlan& r = run.plan;
  hipStream_t st = run.st;
  // eCoherentRR: a vertex shaded in round `depth` has path_length depth + 2; the roulette runs for
  // gMinPathVertices <= path_length < gMaxPathVertices at a non-specular vertex that is within the diffuse budget —
  // without specular materials that is vertex number depth + 1 of at most gMaxDiffuseVertices. In such a round the
  // paths first report their p (k_shade<PROBE>), the 8x4 groups agree (k_rr_reduce), then the round proper runs.
  // A probe: the round's k_shade without any output, up to the statement `kind` names (FrameParams::probe_kind)
  auto launch_probe = [&](uint32_t kind) {
    FrameParams probe = p;
    probe.probe_kind = kind;
    probe.out_albedo = nullptr;
    probe.out_visibility = nullptr;
    probe.out_depth = nullptr;
    probe.out_prev_uv = nullptr;
    launch_kernel(r.k_probe, r.grid, r.probe_lds, st, probe, depth);
  };
  const unsigned reduce_grid = (unsigned)((p.path_count + STHIP_BLOCK - 1) / STHIP_BLOCK);
  const bool any_paths = p.path_count != 0;  // a shard that owns no tile of a small frame has no path: nothing to probe or reduce (and no grid of 0 blocks)
  p.rr = nullptr;
  if (any_paths && r.coherent_rr && depth + 2 >= r.pc.gMinPathVertices && depth + 2 < r.pc.gMaxPathVertices && (ctx->has_specular || depth + 1 <= r.pc.gMaxDiffuseVertices)) {
    p.rr = ctx->rr.p;
    (void)hipMemsetAsync(ctx->rr.p, 0, (size_t)p.path_count * 16, st);
    launch_probe(1);
    hipLaunchKernelGGL(k_rr_reduce, dim3(reduce_grid), dim3(STHIP_BLOCK), 0, st, p);
  }
  // eCoherentSampling: the NEE index first (with the roulette's verdict known), then connect_lvc's (with the NEE index
  // known: how many numbers a path draws in between depends on the candidates it looked at)
  p.cs_nee = nullptr;
  p.cs_lvc = nullptr;
  if (any_paths && r.coherent_nee) {
    p.cs_nee = ctx->cs_nee.p;
    (void)hipMemsetAsync(ctx->cs_nee.p, 0, (size_t)p.path_count * 8, st);
    launch_probe(2);
    hipLaunchKernelGGL(k_cs_reduce, dim3(reduce_grid), dim3(STHIP_BLOCK), 0, st, p.cs_nee, p.path_count);
  }
  if (any_paths && r.coherent_lvc) {
    p.cs_lvc = ctx->cs_lvc.p;
    (void)hipMemsetAsync(ctx->cs_lvc.p, 0, (size_t)p.path_count * 8, st);
    launch_probe(3);
    hipLaunchKernelGGL(k_cs_reduce, dim3(reduce_grid), dim3(STHIP_BLOCK), 0, st, p.cs_lvc, p.path_count);
  }
  // untextured scenes, no light subpaths, no media, no debug mode. Where the path or diffuse budget can end at this round's
  // vertex, only the paths that still have something to do reach k_shade (k_cull_terminal).
  const bool plain = !ctx->textured && !r.bdpt && !r.media && !r.debug_mode;
  if (plain && ctx->cull_terminal && depth >= 1 && !p.rr && !p.cs_nee && !p.cs_lvc && (depth + 2 >= r.pc.gMaxPathVertices || depth + 1 > r.pc.gMaxDiffuseVertices)) {
    // a block keeps what it meets in LDS: as many blocks per segment as it takes for a segment's share to fit (16 KB at 1080p)
    uint32_t per_segment = CULL_BLOCKS_PER_SEGMENT, per_block;
    for (;; per_segment *= 2) {
      per_block = (uint32_t)((((size_t)p.seg_stride + (size_t)per_segment * STHIP_BLOCK - 1) / ((size_t)per_segment * STHIP_BLOCK)) * STHIP_BLOCK);  // entries a block can meet
      if ((size_t)(per_block + 2) * 4 <= 48 * 1024) break;
    }
    hipLaunchKernelGGL(k_cull_terminal, dim3(QUEUE_SEGMENTS * per_segment), dim3(STHIP_BLOCK), (size_t)(per_block + 2) * 4, st, p, depth, ctx->queue_kept.p, per_block);
    FrameParams pk = p;
    pk.queue[depth & 1u] = ctx->queue_kept.p;
    pk.culled = 1;
    launch_kernel(r.k_shade, r.grid, r.shade_lds, st, pk, depth);
  } else {
    launch_kernel(r.k_shade, r.grid, r.shade_lds, st, p, depth);
  }
}

// The passes of every batch of seeds: the light pass (sample_photons), the compaction of the light vertex cache, the view pass,
// k_resolve, and the hash grids the next seed looks into
static int run_batches(const RenderRun& run, FrameParams& p, uint32_t seed_begin, uint32_t seed_count) {
  sthip_ctx* ctx = run.ctx;
  const RenderPlan& r = run.plan;
  const sthip_BDPTPushConstants* pc = &r.pc;
  hipStream_t st = run.st;
  const uint32_t grid = r.grid;
  const size_t pixels = r.pixels, hg_slots = r.hg_slots;
  const bool timing = ctx->time_kernels;
  float ms_trace = 0, ms_primary = 0, ms_shade = 0, ms_other = 0;
  uint32_t launches_trace = 0, launches_primary = 0;
  uint64_t rays_primary = 0;
  auto timed = [&](float& acc, auto&& launch) -> int {
    if (timing) HIP_TRY(ctx, hipEventRecord(ctx->ev[0], st));
    launch();
    HIP_TRY(ctx, hipGetLastError());
    if (timing) {
      HIP_TRY(ctx, hipEventRecord(ctx->ev[1], st));
      HIP_TRY(ctx, hipEventSynchronize(ctx->ev[1]));
      float ms = 0;
      HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
      acc += ms;
    }
    return STHIP_OK;
  };
  bool counters_cleared = false;  // (the first pass's k_clear takes the counters along with its queue control words)
  for (uint32_t s = 0; s < seed_count; s += r.batch) {
    const uint32_t in_flight = std::min(r.batch, seed_count - s);
    p.seed = seed_begin + s;
    p.seeds_in_flight = in_flight;
    p.write_aov = s == 0 ? 1u : 0u;
    int rc = STHIP_OK;
    // queue sizes and heads are per pass; the ray / traversal counters run over the whole call
    auto reset_queues = [&]() -> int {
      const uint32_t per_depth = QUEUE_SEGMENTS * QCTL_STRIDE;  // 64-bit words
      const uint32_t words = (r.max_bounce_rounds + r.drain_rounds + 1) * per_depth;  // the last round's shade appends to depth + 1; k_resolve sums p.rounds of them
      hipLaunchKernelGGL(k_clear, dim3(std::max(1u, std::min(64u, (2 * words + CNT_TOTAL + STHIP_BLOCK - 1) / STHIP_BLOCK))), dim3(STHIP_BLOCK), 0, st, queue_ctl_host(ctx->qctl.p, 0, 0), words,
                         queue_ctl_host(ctx->qctl.p, 1, 0), words, ctx->counters.p, counters_cleared ? 0u : (uint32_t)CNT_TOTAL);
      counters_cleared = true;
      if (p.shadow_debug) HIP_TRY(ctx, hipMemsetAsync(queue_ctl_host(ctx->qctl.p, 2, 0), 0, (size_t)words * 8, st));  // the debug halves' queues (BDPTDebugMode)
      HIP_TRY(ctx, hipGetLastError());
      return STHIP_OK;
    };
    auto trace = [&](uint32_t dc, uint32_t ds) -> int {
      if (dc == TRACE_NONE && ds == TRACE_NONE) return STHIP_OK;
      launches_trace++;
      return timed(ms_trace, [&]() {
        launch_trace(run, p, dc, ds, ctx->count_traversal);
        if (p.shadow_debug && ds != TRACE_NONE) {
          // BDPTDebugMode: the same shadow rays once more, carrying what each adds to the debug image, accumulated into the paths'
          // debug pixels the way the first pass accumulated their contributions into the radiance (finish_ray)
          FrameParams q = p;
          q.shadow_rays = p.shadow_debug;
          q.radiance = p.debug;
          q.shadow_sum = p.debug;  // (a connection's debug half exists while NEE's rays are deferred: finish_ray's target either way)
          q.qctl = p.qctl + (size_t)64 * QUEUE_SEGMENTS * QCTL_STRIDE;  // its "shadow queues" (kind 1) are the debug queues (kind 2) k_shade filled
          launch_trace(run, q, TRACE_NONE, ds, false);
        }
      });
    };
    // the first bounce as wave packets (k_trace_primary): one 8x8 pixel block per wave, over the first `seeds` seeds in flight of `q`
    auto launch_primary = [&](const FrameParams& q, uint32_t seeds) -> int {
      launches_primary++;
      rays_primary += (uint64_t)r.primary_rays * seeds;
      const uint32_t packets = (q.path_count + 63) / 64;
      const unsigned pgrid = std::max(1u, std::min((packets + 3) / 4, (uint32_t)ctx->cu_count * 64u));
      const size_t plds = ((size_t)ctx->bvh.stack_depth * (STHIP_BLOCK / 64) + 13 * STHIP_BLOCK) * sizeof(uint32_t);  // the per-wave stacks + every lane's saved world-space ray constants
      return timed(ms_primary, [&]() { launch_kernel(STHIP_KERNEL2(k_trace_primary, ctx->count_traversal, q.bvh.alpha_test != 0), pgrid, plds, st, q); });
    };
    // "reuse_first_hits" (first_hits.h): the hits of the first bounce are those of seed 0's slots for every seed, and for every
    // call of the same key. They are traced into the context's kept buffers, once per change of key (slots are seed x
    // paths_per_seed + pixel slot, and k_generate has written every seed's rays by now: seed 0's are as good as any). With one
    // seed in flight round 0 is shaded straight from the kept buffers (shade_first_round); with several, a streaming kernel
    // writes the kept hits to every seed's slots of p.hit / p.hit_leaf.
    const bool from_kept = r.keep_first_hits;
    auto trace_primary = [&]() -> int {
      if (!from_kept) return launch_primary(p, in_flight);
      if (!(ctx->first_hits_valid && sthip::first_hit_key_equal(ctx->first_hit_key, r.first_hit_key))) {
        ctx->first_hits_valid = false;
        FrameParams q = p;
        q.path_count = p.paths_per_seed;
        q.hit = ctx->first_hit.p;
        q.hit_leaf = ctx->first_hit_leaf.p;
        const int e = launch_primary(q, 1);
        if (e) return e;
        ctx->first_hit_key = r.first_hit_key;  // (valid only now that the launch that fills them is enqueued)
        ctx->first_hits_valid = true;
      }
      if (in_flight > 1)
        return timed(ms_primary, [&]() {
          hipLaunchKernelGGL(k_replicate_first_hits, dim3(grid_for(ctx, p.paths_per_seed)), dim3(STHIP_BLOCK), 0, st, (const float4*)ctx->first_hit.p, (const uint32_t*)ctx->first_hit_leaf.p, p.hit,
                             p.hit_leaf, p.paths_per_seed, in_flight);
        });
      return STHIP_OK;
    };
    // round 0 of the view pass: its hits are the kept ones where they were not copied (k_shade and its probes are their only
    // readers: k_cull_terminal runs from round 1 on, and k_trace writes p.hit afresh for every later round)
    auto shade_first_round = [&]() {
      FrameParams q = p;
      q.hit = ctx->first_hit.p;
      q.hit_leaf = ctx->first_hit_leaf.p;
      shade_view_round(run, q, 0);
    };
    // Round r traces the paths entering bounce r together with the shadow rays bounce r - 1 produced (one launch,
    // k_trace), then shades bounce r; a last launch traces the shadow rays of the last bounce. `shade(depth)` is the
    // pass's shading kernel; the light pass (sample_photons) has visibility rays to the camera in place of NEE rays.
    auto run_rounds = [&](bool light, bool shadow_rays, auto&& shade) -> int {
      for (uint32_t depth = 0; depth <= r.max_bounce_rounds; depth++) {
        const uint32_t dc = depth < r.max_bounce_rounds ? depth : TRACE_NONE;
        const uint32_t ds = depth >= 1 && shadow_rays && depth - 1 <= r.max_shadow_round ? depth - 1 : TRACE_NONE;
        int e;
        if (!light && depth == 0 && dc == 0 && ctx->packet_primary && !ctx->has_volumes) {
          e = trace_primary();
        } else if (ctx->fuse_trace) {
          e = trace(dc, ds);
        } else {  // analysis: the two ray kinds in launches of their own
          e = trace(TRACE_NONE, ds);
          if (!e) e = trace(dc, TRACE_NONE);
        }
        if (e) return e;
        if (r.media && ds != TRACE_NONE) {
          e = timed(ms_shade, [&]() { hipLaunchKernelGGL(k_shadow_media, dim3(grid), dim3(STHIP_BLOCK), 0, st, p, ds); });
          if (e) return e;
        }
        if (dc == TRACE_NONE) break;
        e = timed(ms_shade, [&]() { shade(depth); });
        if (e) return e;
      }
      if (r.media && shadow_rays)  // the shadow rays still walking after the last bounce
        for (uint32_t ds = r.max_bounce_rounds; ds < r.max_bounce_rounds + r.drain_rounds; ds++) {
          int e = trace(TRACE_NONE, ds);
          if (!e) e = timed(ms_shade, [&]() { hipLaunchKernelGGL(k_shadow_media, dim3(grid), dim3(STHIP_BLOCK), 0, st, p, ds); });
          if (e) return e;
        }
      return STHIP_OK;
    };

    if (r.connect_paths) {  // BDPT.cpp:655-659; `conn` holds no pending entries when a pass starts
      HIP_TRY(ctx, hipMemsetAsync(ctx->light_vertices.p, 0, std::max<size_t>(1, r.vertices_per_seed * in_flight) * 64, st));
      if (r.lvc) HIP_TRY(ctx, hipMemsetAsync(ctx->lvc_staging.p, 0, (size_t)in_flight * pc->gLightPathCount * (pc->gMaxDiffuseVertices - 1) * 64, st));
      if (p.conn) HIP_TRY(ctx, hipMemsetAsync(ctx->conn.p, 0, (size_t)in_flight * p.paths_per_seed * r.conn_per_path * 16, st));
    }
    if (r.light_tracing) {  // sample_photons before the view paths, BDPT.cpp:653-667
      if (r.connect_views) HIP_TRY(ctx, hipMemsetAsync(ctx->light_trace.p, 0, (size_t)in_flight * r.W * r.H * 16, st));
      p.light_pass = 1;
      p.path_count = in_flight * r.light_threads;
      rc = reset_queues();
      if (rc) return rc;
      rc = timed(ms_other, [&]() { launch_kernel(ctx->textured ? (const void*)&k_generate_light<true, true> : (const void*)&k_generate_light<false, true>, grid_for(ctx, p.path_count), 0, st, p); });
      if (rc) return rc;
      rc = run_rounds(true, !r.media, [&](uint32_t depth) { launch_kernel(r.k_shade_light, grid, 0, st, p, depth); });  // (media: connect_view walks its ray itself: nothing is queued)
      if (rc) return rc;
      rc = timed(ms_other, [&]() { hipLaunchKernelGGL(k_count_rays, dim3(1), dim3(1), 0, st, p); });
      if (rc) return rc;
      p.light_pass = 0;
    }
    if (r.lvc) {  // the cache in its defined order: compact the staged vertices of every seed in flight (lvc.hip)
      const uint32_t slots_per_seed = pc->gLightPathCount * (pc->gMaxDiffuseVertices - 1);
      size_t tmp_bytes = ctx->lvc_tmp.n;
      if (r.light_tracing)
        HIP_TRY(ctx, sthip::lvc_compact(ctx->lvc_staging.p, slots_per_seed, in_flight, (uint32_t)r.vertices_per_seed, ctx->light_vertices.p, ctx->lvc_count.p, ctx->lvc_flags.p, ctx->lvc_offsets.p,
                                        ctx->lvc_tmp.p, tmp_bytes, st));
      else
        HIP_TRY(ctx, hipMemsetAsync(ctx->lvc_count.p, 0, (size_t)in_flight * 4, st));
    }

    if (r.nee_reuse) HIP_TRY(ctx, hipMemsetAsync(ctx->hg_appends.p, 0, hg_slots * 64, st));
    if (r.lvc_reuse) HIP_TRY(ctx, hipMemsetAsync(ctx->lg_appends.p, 0, hg_slots * 96, st));
    p.path_count = in_flight * p.paths_per_seed;
    rc = reset_queues();
    if (rc) return rc;
    rc = timed(ms_other, [&]() { hipLaunchKernelGGL(k_generate, dim3(grid), dim3(STHIP_BLOCK), 0, st, p); });
    if (rc) return rc;
    if (r.debug_mode == STHIP_DEBUG_ENVIRONMENT_SAMPLE_TEST || r.debug_mode == STHIP_DEBUG_ENVIRONMENT_SAMPLE_PDF) {
      // bdpt.hlsl:190-205: sample_visibility returns before it traces anything; the frame stays (0, 0, 0, 1), no ray is counted
      // (the G-buffer outputs are not written upstream either: they are left zero here)
      if (s == 0) {
        if (p.out_albedo) HIP_TRY(ctx, hipMemsetAsync(p.out_albedo, 0, pixels * 16, st));  // (the binary32 stage with half colour precision)
        if (p.out_visibility) HIP_TRY(ctx, hipMemsetAsync(p.out_visibility, 0, pixels * 8, st));
        if (p.out_depth) HIP_TRY(ctx, hipMemsetAsync(p.out_depth, 0, pixels * 16, st));
        if (p.out_prev_uv) HIP_TRY(ctx, hipMemsetAsync(p.out_prev_uv, 0, pixels * 8, st));
      }
      rc = timed(ms_other, [&]() {
        hipLaunchKernelGGL(k_debug_environment, dim3(grid), dim3(STHIP_BLOCK), 0, st, p);
        hipLaunchKernelGGL(k_resolve, dim3(grid), dim3(STHIP_BLOCK), 0, st, p, s == 0 ? 1u : 0u, s + in_flight == seed_count ? 1u : 0u, 0u);
      });
      if (rc) return rc;
      rays_primary = 0;
      continue;
    }
    if (r.presample) {
      const unsigned pgrid = (unsigned)((r.presample_n * in_flight + STHIP_BLOCK - 1) / STHIP_BLOCK);
      rc = timed(ms_other, [&]() { launch_kernel(STHIP_KERNEL2(k_presample_lights, ctx->textured, ctx->has_spheres || r.has_env), pgrid, 0, st, p); });
      if (rc) return rc;
    }
    p.emitter_count = ctx->answer_last_rays ? ctx->emitter_count : 0u;  // (only the plain k_shade instantiation looks at it)
    rc = run_rounds(false, (r.nee || r.connect_paths) && !r.inline_media, [&](uint32_t depth) {  // (inline walks through media: nothing is queued)
      if (depth == 0 && from_kept && in_flight == 1)
        shade_first_round();
      else
        shade_view_round(run, p, depth);
    });
    if (rc) return rc;
    rc = timed(ms_other, [&]() { hipLaunchKernelGGL(k_resolve, dim3(grid), dim3(STHIP_BLOCK), 0, st, p, s == 0 ? 1u : 0u, s + in_flight == seed_count ? 1u : 0u, r.primary_rays * in_flight); });
    if (rc) return rc;
    if ((r.nee_reuse || r.lvc_reuse) && (s + in_flight < seed_count || ctx->reuse_persist)) {
      // This seed's appends become the grids the next seed looks up (hashgrid.h)
      if (r.nee_reuse) {
        const int rc2 = build_hash_grid(ctx, st, ctx->hg_appends.p, ctx->hg_compact.p, ctx->hg_data.p, hg_slots, 4, 2, false, pc->gHashGridBucketCount, ctx->hg_checksums, ctx->hg_counters, ctx->hg_indices);
        if (rc2) return rc2;
      }
      if (r.lvc_reuse) {
        const int rc2 = build_hash_grid(ctx, st, ctx->lg_appends.p, ctx->lg_compact.p, ctx->lg_data.p, hg_slots, 6, 0, true, pc->gHashGridBucketCount, ctx->lg_checksums, ctx->lg_counters, ctx->lg_indices);
        if (rc2) return rc2;
      }
      p.hg_prev = 1;
    }
  }
  if (timing) {
    ctx->stats.ms_trace = ms_trace;
    ctx->stats.ms_shade = ms_shade;
    ctx->stats.ms_total = ms_trace + ms_primary + ms_shade + ms_other;
    ctx->stats.launches_trace = launches_trace;
    ctx->stats.ms_trace_primary = ms_primary;
    ctx->stats.launches_primary = launches_primary;
  }
  ctx->stats.rays_primary_packets = rays_primary;
  return STHIP_OK;
}

// The staged images to the caller's host memory, on stream `s` (the render stream, or the copy stream of the pipelined form)
static int read_back(sthip_ctx* ctx, const RenderPlan& r, const FrameParams& p, const sthip_outputs* out, hipStream_t s) {
  const size_t pixels = r.pixels, cb = ctx->color_bytes();
  HIP_TRY(ctx, hipMemcpyAsync(out->gRadiance, p.out_radiance, r.radiance_entries * cb, hipMemcpyDeviceToHost, s));
  if (out->gAlbedo) HIP_TRY(ctx, hipMemcpyAsync(out->gAlbedo, p.out_albedo16 ? (const void*)p.out_albedo16 : (const void*)p.out_albedo, pixels * cb, hipMemcpyDeviceToHost, s));
  if (out->gVisibility) HIP_TRY(ctx, hipMemcpyAsync(out->gVisibility, p.out_visibility, pixels * 8, hipMemcpyDeviceToHost, s));
  if (out->gDepth) HIP_TRY(ctx, hipMemcpyAsync(out->gDepth, p.out_depth, pixels * 16, hipMemcpyDeviceToHost, s));
  if (out->gPrevUVs) HIP_TRY(ctx, hipMemcpyAsync(out->gPrevUVs, p.out_prev_uv, pixels * 8, hipMemcpyDeviceToHost, s));
  return STHIP_OK;
}

// One attempt at a render call. `slot`: the frame of sthip_render_async whose staging set and events the call uses (nullptr:
// the synchronous form).
static int render_once(sthip_ctx* ctx, const sthip_BDPTPushConstants* pc, uint32_t sampling_flags, uint32_t scene_flags, const sthip_frame_desc* frame, uint32_t seed_begin, uint32_t seed_count,
                       const sthip_outputs* out, AsyncSlot* slot) {
  RenderPlan plan;
  int rc = plan_render(ctx, pc, sampling_flags, scene_flags, frame, seed_count, out, plan);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  rc = reserve_render_buffers(ctx, plan, out, slot);
  if (rc) return rc;
  FrameParams p;
  rc = bind_frame_params(ctx, plan, frame, out, slot, p);
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  RenderRun run{ctx, plan, st, 0, trace_lds_bytes(ctx)};
  run.tgrid = std::min<uint32_t>(trace_grid(ctx, run.lds), (uint32_t)((plan.P + STHIP_BLOCK - 1) / STHIP_BLOCK));
  if (ctx->bvh.spill) run.tgrid = std::min<uint32_t>(run.tgrid, (uint32_t)ctx->cu_count * 8u);  // what the spill buffer has columns for (configure_stack)

  ctx->render_launched = true;  // everything the call needs is allocated: from here on work is enqueued
  // the deep queue's control words: k_trace_deep leaves them at zero, but a call that was cut short between k_trace and
  // k_trace_deep (a failed launch, an error return) would not have: one 8-byte fill per call keeps every call self-contained
  if (ctx->bvh.spill && ctx->deep_count.p) HIP_TRY(ctx, hipMemsetAsync(ctx->deep_count.p, 0, 8, st));
  rc = run_batches(run, p, seed_begin, seed_count);
  if (rc) return rc;
  if ((plan.nee_reuse || plan.lvc_reuse) && ctx->reuse_persist) {  // what the next call's first seed may look into
    memcpy(ctx->reuse_key, plan.reuse_key, sizeof plan.reuse_key);
    ctx->reuse_grids_valid = true;
  }

  if (slot) {
    // The read-back of the pipelined form: on the copy stream, behind the "rendered" event, so that the runtime moves this frame
    // (a copy engine, or its copy kernel on a hardware queue of its own: ~0.6 ms per 33 MB image) while the next one is traced. ctx->counters is rewritten by the next frame's k_clear: its read-out into
    // the slot is a device-to-device copy ON THE RENDER STREAM, ordered before that rewrite; the copy stream then takes the
    // slot's counters to the pinned record. Nothing waits on the host, nothing spins on the device: events only.
    hipStream_t cs = ctx->copy_stream;
    HIP_TRY(ctx, hipMemcpyAsync(slot->counters.p, ctx->counters.p, CNT_TOTAL * sizeof(unsigned long long), hipMemcpyDeviceToDevice, st));
    HIP_TRY(ctx, hipEventRecord(slot->rendered, st));
    HIP_TRY(ctx, hipStreamWaitEvent(cs, slot->rendered, 0));
    rc = read_back(ctx, plan, p, out, cs);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(slot->record, slot->counters.p, CNT_TOTAL * sizeof(unsigned long long), hipMemcpyDeviceToHost, cs));
    HIP_TRY(ctx, hipEventRecord(slot->copied, cs));
    slot->ray_count = out->gRayCount;
    ctx->stats_pending = true;  // (until the ticket is retired, sthip_get_stats reads the counters of the last frame enqueued)
  } else if (!plan.dev) {
    rc = read_back(ctx, plan, p, out, st);
    if (rc) return rc;
    if (plan.debug_mode) HIP_TRY(ctx, hipMemcpyAsync(out->gDebugImage, p.out_debug, plan.pixels * ctx->color_bytes(), hipMemcpyDeviceToHost, st));
    unsigned long long c[CNT_TOTAL];
    HIP_TRY(ctx, hipMemcpyAsync(c, ctx->counters.p, sizeof(c), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (out->gRayCount) {
      out->gRayCount[0] = c[CNT_RAYS_CLOSEST] + c[CNT_RAYS_SHADOW];
      out->gRayCount[1] = c[CNT_RAYS_CLOSEST] - c[CNT_CROSSINGS];
    }
    fill_counter_stats(ctx, c);
    ctx->stats_pending = false;
  } else {
    if (out->gRayCount) hipLaunchKernelGGL(k_write_ray_count, dim3(1), dim3(1), 0, st, ctx->counters.p, reinterpret_cast<unsigned long long*>(out->gRayCount));
    ctx->stats_pending = true;
  }
  return STHIP_OK;
}

// A render allocates its path state (~330 B per path in flight at the default flags) before it enqueues anything. Should the
// device not have that much left — a host application that holds memory of its own, several contexts on one device — the
// batch is halved (fewer seeds traced together: the same frame, a little slower) and the call tried again, down to one seed;
// the smaller batch stays for the calls that follow (stats: max_paths_in_flight, batch_halvings).
static int render_with_retry(sthip_ctx* ctx, const sthip_BDPTPushConstants* pc, uint32_t sampling_flags, uint32_t scene_flags, const sthip_frame_desc* frame, uint32_t seed_begin, uint32_t seed_count,
                             const sthip_outputs* out, AsyncSlot* slot) {
  for (;;) {
    ctx->last_hip_error = hipSuccess;
    ctx->render_launched = false;
    const int rc = render_once(ctx, pc, sampling_flags, scene_flags, frame, seed_begin, seed_count, out, slot);
    ctx->stats.max_paths_in_flight = ctx->max_paths_in_flight;
    if (rc != STHIP_ERR_HIP || ctx->last_hip_error != hipErrorOutOfMemory || ctx->render_launched) return rc;
    (void)hipGetLastError();  // (the allocation's error is not sticky, but it is the "last error" until read)
    const uint64_t per_seed = std::max<uint64_t>(1, ctx->stats.paths_per_seed);
    if (ctx->max_paths_in_flight <= per_seed || ctx->max_paths_in_flight <= 1) return rc;  // one seed in flight already: it does not fit
    (void)drain_in_flight(ctx);  // (frames of sthip_render_async: complete before the state they were traced with goes)
    release_path_state(ctx);
    ctx->max_paths_in_flight = std::max<uint64_t>(per_seed, ctx->max_paths_in_flight / 2);
    ctx->stats.batch_halvings++;
    if (getenv("STHIP_VERBOSE")) fprintf(stderr, "[sthip] out of device memory (%s): max_paths_in_flight -> %llu\n", ctx->error.c_str(), (unsigned long long)ctx->max_paths_in_flight);
  }
}

int sthip_render(sthip_ctx* ctx, const sthip_BDPTPushConstants* pc, uint32_t sampling_flags, uint32_t scene_flags, const sthip_frame_desc* frame, uint32_t seed_begin,
                 uint32_t seed_count, const sthip_outputs* out) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  return render_with_retry(ctx, pc, sampling_flags, scene_flags, frame, seed_begin, seed_count, out, nullptr);
}

// ---- pipelined host outputs (sthip.h: sthip_render_async) ----

int sthip_host_alloc(sthip_ctx* ctx, uint64_t bytes, void** out) {
  if (!ctx || !out) return STHIP_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (bytes == 0) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_host_alloc: 0 bytes");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  void* q = nullptr;
  HIP_TRY(ctx, hipHostMalloc(&q, (size_t)bytes, hipHostMallocDefault));
  ctx->host_allocs.push_back(q);
  *out = q;
  return STHIP_OK;
}

int sthip_host_free(sthip_ctx* ctx, void* p) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  if (!p) return STHIP_OK;
  const auto it = std::find(ctx->host_allocs.begin(), ctx->host_allocs.end(), p);
  if (it == ctx->host_allocs.end()) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_host_free: not a pointer of sthip_host_alloc");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, drain_in_flight(ctx));  // a frame in flight may still copy into it
  ctx->host_allocs.erase(it);
  HIP_TRY(ctx, hipHostFree(p));
  return STHIP_OK;
}

int sthip_render_async(sthip_ctx* ctx, const sthip_BDPTPushConstants* pc, uint32_t sampling_flags, uint32_t scene_flags, const sthip_frame_desc* frame, uint32_t seed_begin,
                       uint32_t seed_count, const sthip_outputs* out, uint64_t* ticket) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  if (!ticket || !out) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render_async: outputs or ticket is NULL");
  *ticket = 0;
  if (out->device_ptrs) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "render_async: device_ptrs must be 0 (sthip_render with device pointers only enqueues already)");
  if (out->debug_mode != 0) return fail(ctx, STHIP_ERR_UNSUPPORTED, "render_async: debug_mode != 0 (gDebugImage chains from frame to frame through host memory): use sthip_render");
  if (ctx->time_kernels) return fail(ctx, STHIP_ERR_UNSUPPORTED, "render_async: \"time_kernels\" = 1 (its events synchronise the host): use sthip_render");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->copy_stream) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
  while (ctx->ring.size() < ctx->output_ring) {
    AsyncSlot* s = new AsyncSlot();
    hipError_t e = hipEventCreateWithFlags(&s->rendered, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->copied, hipEventDisableTiming);
    if (e == hipSuccess) e = hipHostMalloc((void**)&s->record, CNT_TOTAL * sizeof(unsigned long long), hipHostMallocDefault);
    if (e != hipSuccess) delete s;  // (a slot is whole or absent)
    HIP_TRY(ctx, e);
    ctx->ring.push_back(s);
  }
  const uint64_t t = ctx->next_ticket;
  AsyncSlot* slot = slot_of(ctx, t);
  // The ring is full: the oldest frame in flight owns this slot. Its COPY is waited for (the slot's pinned blocks and staging
  // set are about to be rewritten). Its ticket is NOT retired: what the host still owes it — gRayCount, the stats — moves to
  // ctx->finished until the caller waits for it.
  if (slot->ticket) {
    HIP_TRY(ctx, hipEventSynchronize(slot->copied));
    sthip_ctx::FinishedFrame& f = ctx->finished[slot->ticket];
    f.counters.assign(slot->record, slot->record + CNT_TOTAL);
    f.ray_count = slot->ray_count;
    slot->ticket = 0;
    slot->ray_count = nullptr;
  }
  const int rc = render_with_retry(ctx, pc, sampling_flags, scene_flags, frame, seed_begin, seed_count, out, slot);
  if (rc != STHIP_OK) return rc;
  slot->ticket = t;
  ctx->next_ticket = t + 1;
  *ticket = t;
  return STHIP_OK;
}

int sthip_outputs_ready(sthip_ctx* ctx, uint64_t ticket) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  if (ticket == 0 || ticket >= ctx->next_ticket) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "outputs_ready: no such ticket");
  if (ticket <= ctx->retired) return 1;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  AsyncSlot* s = slot_of(ctx, ticket);
  const hipError_t e = s->ticket == ticket ? hipEventQuery(s->copied) : hipSuccess;  // (not in its slot any more: completed when the slot was taken over)
  if (e == hipErrorNotReady) return 0;
  HIP_TRY(ctx, e);
  retire_through(ctx, ticket);  // (the copy stream runs the frames in submission order: the earlier ones are complete too)
  return 1;
}

int sthip_wait_outputs(sthip_ctx* ctx, uint64_t ticket) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  if (ticket == 0 || ticket >= ctx->next_ticket) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "wait_outputs: no such ticket");
  if (ticket <= ctx->retired) return STHIP_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, complete_ticket(ctx, ticket));
  retire_through(ctx, ticket);
  return STHIP_OK;
}

// ---- multi-GPU assembly: the packed tiles of every shard -> the frame ----

uint32_t sthip_shard_slot_count(uint32_t width, uint32_t height, uint32_t shard_rank, uint32_t shard_count, uint32_t tile_w, uint32_t tile_h) {
  if (!width || !height || !shard_count || !tile_w || !tile_h || shard_rank >= shard_count) return 0;
  const uint32_t tiles = ((width + tile_w - 1) / tile_w) * ((height + tile_h - 1) / tile_h);
  return owned_tiles(tiles, shard_rank, shard_count) * tile_w * tile_h;
}

int sthip_assemble_tiles_bytes(sthip_ctx* ctx, const void* packed, uint64_t rank_stride, uint32_t shard_count, uint32_t tile_w, uint32_t tile_h, uint32_t width, uint32_t height,
                               uint32_t entry_bytes, void* frame) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  if (!packed || !frame || !shard_count || !width || !height) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_assemble_tiles: a required argument is NULL/zero");
  if (tile_w == 0 || tile_h == 0 || (tile_w & 7) || (tile_h & 7)) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_assemble_tiles: tile size must be a multiple of 8");
  if (entry_bytes == 0 || entry_bytes > 64 || (entry_bytes & 3)) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_assemble_tiles: entry size must be a multiple of 4 bytes, at most 64");
  const uint32_t slots = sthip_shard_slot_count(width, height, 0, shard_count, tile_w, tile_h);  // rank 0 owns the most tiles
  if (rank_stride < slots) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_assemble_tiles: rank_stride is smaller than a shard's slot count");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)shard_count * slots;
  hipLaunchKernelGGL(k_assemble_tiles, dim3((unsigned)((n + STHIP_BLOCK - 1) / STHIP_BLOCK)), dim3(STHIP_BLOCK), 0, ctx->stream, reinterpret_cast<const uint32_t*>(packed), (size_t)rank_stride, shard_count,
                     slots, tile_w, tile_h, width, height, entry_bytes / 4, reinterpret_cast<uint32_t*>(frame));
  HIP_TRY(ctx, hipGetLastError());
  return STHIP_OK;
}
int sthip_assemble_tiles(sthip_ctx* ctx, const float* packed, uint64_t rank_stride, uint32_t shard_count, uint32_t tile_w, uint32_t tile_h, uint32_t width, uint32_t height,
                         float* frame) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  return sthip_assemble_tiles_bytes(ctx, packed, rank_stride, shard_count, tile_w, tile_h, width, height, (uint32_t)ctx->color_bytes(), frame);
}
int sthip_radiance_to_sums(sthip_ctx* ctx, float* image, uint64_t entries, uint32_t back) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  if (!image) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_radiance_to_sums: image is NULL");
  if (ctx->half_color) return fail(ctx, STHIP_ERR_UNSUPPORTED, "sthip_radiance_to_sums: not with half_color_precision (a sum of rounded means is not a rounded mean)");
  if (entries == 0) return STHIP_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_radiance_sums, dim3(grid_for(ctx, (size_t)entries)), dim3(STHIP_BLOCK), 0, ctx->stream, reinterpret_cast<float4*>(image), (size_t)entries, back ? 0u : 1u);
  HIP_TRY(ctx, hipGetLastError());
  return STHIP_OK;
}

int sthip_pack_tiles(sthip_ctx* ctx, const void* image, uint32_t width, uint32_t height, uint32_t entry_bytes, void* packed) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  if (!image || !packed || !width || !height) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_pack_tiles: a required argument is NULL/zero");
  if (entry_bytes == 0 || entry_bytes > 64 || (entry_bytes & 3)) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_pack_tiles: entry size must be a multiple of 4 bytes, at most 64");
  const uint32_t slots = sthip_shard_slot_count(width, height, ctx->shard_rank, ctx->shard_count, ctx->tile_w, ctx->tile_h);
  if (slots == 0) return STHIP_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_pack_tiles, dim3((unsigned)((slots + STHIP_BLOCK - 1) / STHIP_BLOCK)), dim3(STHIP_BLOCK), 0, ctx->stream, reinterpret_cast<const uint32_t*>(image), ctx->shard_rank, ctx->shard_count,
                     slots, ctx->tile_w, ctx->tile_h, width, height, entry_bytes / 4, reinterpret_cast<uint32_t*>(packed));
  HIP_TRY(ctx, hipGetLastError());
  return STHIP_OK;
}

}  // extern "C"
