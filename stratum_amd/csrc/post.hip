// post.hip — the calls of the C ABI (include/sthip.h) after the path and beside it: temporal accumulation, the denoiser's
// filter, material conversion, the density grid of a dense box, tonemap and image metric, and the measured ceilings of the
// roofline.
#include "ceilings.h"
#include "context.h"
#include "denoise.h"
#include "material_convert.h"
#include "post.h"
#include "texel_decode.h"

// ---- after the path: temporal accumulation, tonemap and image metric (post.h) ----

int sthip_accumulate(sthip_ctx* ctx, const sthip_accumulate_desc* d) {
  if (!ctx || !d) return STHIP_ERR_INVALID_ARGUMENT;
  if (!d->gViews || !d->view_count || !d->gRadiance || !d->gPrevAccumColor || !d->gPrevAccumMoments || !d->gAccumColor || !d->gAccumMoments || !d->width || !d->height)
    return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_accumulate: gViews, gRadiance, gPrevAccum*, gAccum* and a non-empty extent are required");
  if (d->demodulate_albedo && !d->gAlbedo) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_accumulate: gDemodulateAlbedo needs gAlbedo");
  if (d->reprojection && (!d->gVisibility || !d->gDepth || !d->gPrevUVs || !d->gPrevVisibility || !d->gPrevDepth))
    return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_accumulate: gReprojection needs gVisibility, gDepth, gPrevUVs, gPrevVisibility, gPrevDepth");
  if ((uint64_t)d->width * d->height > 0x7FFFFFFFull) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_accumulate: extent too large");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t n = (size_t)d->width * d->height;
  std::vector<void*> staged;  // device copies of host inputs, freed on return
  auto release = [&]() {
    for (void* q : staged) (void)hipFree(q);
  };
  bool bad = false;
  auto in = [&](const void* host, size_t bytes) -> const void* {
    if (!host || d->device_ptrs) return host;
    void* q = nullptr;
    if (hipMalloc(&q, bytes) != hipSuccess || hipMemcpyAsync(q, host, bytes, hipMemcpyHostToDevice, st) != hipSuccess) {
      bad = true;
      return nullptr;
    }
    staged.push_back(q);
    return q;
  };
  AccumulateParams p{};
  p.width = d->width;
  p.height = d->height;
  p.view_count = d->view_count;
  p.reprojection = d->reprojection;
  p.demodulate_albedo = d->demodulate_albedo;
  p.history_limit = d->history_limit;
  p.instance_count = d->instance_count;
  if (d->view_count <= ACCUMULATE_INLINE_VIEWS) {  // gViews is a host array in either mode: a few views ride in the kernel's arguments
    p.views = nullptr;
    memcpy(p.inline_views, d->gViews, (size_t)d->view_count * sizeof(sthip_ViewData));
  } else {
    void* q = nullptr;
    if (hipMalloc(&q, (size_t)d->view_count * sizeof(sthip_ViewData)) != hipSuccess ||
        hipMemcpyAsync(q, d->gViews, (size_t)d->view_count * sizeof(sthip_ViewData), hipMemcpyHostToDevice, st) != hipSuccess)
      bad = true;
    else
      staged.push_back(q);
    p.views = (const sthip_ViewData*)q;
  }
  const size_t cb = ctx->color_bytes();  // gRadiance, gAlbedo, gPrevAccumColor, gAccumColor
  p.radiance = in(d->gRadiance, n * cb);
  p.albedo = in(d->gAlbedo, n * cb);
  p.visibility = (const sthip_VisibilityInfo*)in(d->gVisibility, n * 8);
  p.depth = (const sthip_DepthInfo*)in(d->gDepth, n * 16);
  p.prev_uvs = (const float2*)in(d->gPrevUVs, n * 8);
  p.prev_visibility = (const sthip_VisibilityInfo*)in(d->gPrevVisibility, n * 8);
  p.prev_depth = (const sthip_DepthInfo*)in(d->gPrevDepth, n * 16);
  p.prev_accum_color = in(d->gPrevAccumColor, n * cb);
  p.prev_accum_moments = (const float2*)in(d->gPrevAccumMoments, n * 8);
  p.instance_index_map = (const uint32_t*)in(d->gInstanceIndexMap, (size_t)d->instance_count * 4);
  void* out_c = d->gAccumColor;
  float2* out_m = reinterpret_cast<float2*>(d->gAccumMoments);
  if (!d->device_ptrs) {
    void *qc = nullptr, *qm = nullptr;
    if (hipMalloc(&qc, n * cb) != hipSuccess || hipMalloc(&qm, n * 8) != hipSuccess) bad = true;
    if (qc) staged.push_back(qc);
    if (qm) staged.push_back(qm);
    out_c = qc;
    out_m = (float2*)qm;
    // pixels outside every view keep what the caller's buffers hold
    if (!bad && (hipMemcpyAsync(qc, d->gAccumColor, n * cb, hipMemcpyHostToDevice, st) != hipSuccess || hipMemcpyAsync(qm, d->gAccumMoments, n * 8, hipMemcpyHostToDevice, st) != hipSuccess)) bad = true;
  }
  if (bad) {
    (void)hipStreamSynchronize(st);
    release();
    return fail(ctx, STHIP_ERR_HIP, "sthip_accumulate: staging the host images on the device failed");
  }
  p.accum_color = out_c;
  p.accum_moments = out_m;
  if (ctx->half_color)
    hipLaunchKernelGGL(k_accumulate<Half4>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p);
  else
    hipLaunchKernelGGL(k_accumulate<float4>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && !d->device_ptrs) {
    e = hipMemcpyAsync(d->gAccumColor, out_c, n * cb, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d->gAccumMoments, out_m, n * 8, hipMemcpyDeviceToHost, st);
  }
  // staged copies must outlive the kernel; with device pointers and inline views nothing is staged: the call is only enqueued
  const hipError_t es = staged.empty() ? hipSuccess : hipStreamSynchronize(st);
  release();
  if (e != hipSuccess || es != hipSuccess) return fail(ctx, STHIP_ERR_HIP, std::string("sthip_accumulate: ") + hipGetErrorString(e != hipSuccess ? e : es));
  return STHIP_OK;
}

// The filter of the denoiser (denoise.hip): estimate_variance, the a-trous passes and the history tap, enqueued in order.
int sthip_denoise_filter(sthip_ctx* ctx, const sthip_denoise_desc* d) {
  if (!ctx || !d) return STHIP_ERR_INVALID_ARGUMENT;
  auto refuse = [&](const char* field, const char* why) { return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, std::string("sthip_denoise_filter: ") + field + " " + why); };
  if (!d->width) return refuse("width", "is 0");
  if (!d->height) return refuse("height", "is 0");
  if ((uint64_t)d->width * d->height > 0x7FFFFFFFull) return refuse("width x height", "is too large (more than 2^31 - 1 pixels)");
  if (!d->view_count) return refuse("view_count", "is 0");
  if (d->iterations < 1 || d->iterations > sthip::DENOISE_MAX_ITERATIONS) return refuse("iterations", "must be 1 .. 8");
  if (d->filter_type >= STHIP_FILTER_TYPE_COUNT) return refuse("filter_type", "must be below 6 (STHIP_FILTER_*)");
  if (!d->gViews) return refuse("gViews", "is NULL");
  if (!d->gVisibility) return refuse("gVisibility", "is NULL");
  if (!d->gDepth) return refuse("gDepth", "is NULL");
  if (!d->gAccumColor) return refuse("gAccumColor", "is NULL");
  if (!d->gAccumMoments) return refuse("gAccumMoments", "is NULL");
  if (!d->gFilterImages[0]) return refuse("gFilterImages[0]", "is NULL");
  if (!d->gFilterImages[1]) return refuse("gFilterImages[1]", "is NULL");
  if (d->gInstanceIndexMap && !d->instance_count) return refuse("instance_count", "is 0 with a gInstanceIndexMap");
  for (uint32_t v = 0; v < d->view_count; v++) {  // the taps are bounded by their view: a view must lie inside the images
    const sthip_ViewData& vw = d->gViews[v];
    if (vw.image_min[0] < 0 || vw.image_min[1] < 0 || vw.image_max[0] > (int64_t)d->width || vw.image_max[1] > (int64_t)d->height)
      return refuse("gViews", ("holds a view that leaves the extent (view " + std::to_string(v) + ")").c_str());
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t n = (size_t)d->width * d->height, cb = ctx->color_bytes();
  const bool tapped = d->history_tap >= 1 && d->history_tap <= d->iterations;
  HIP_TRY(ctx, ctx->denoise_guide.ensure(n));  // (no allocation unless the extent exceeds every earlier call's)
  std::vector<void*> staged;  // device copies of host arrays, freed on return
  auto release = [&]() {
    for (void* q : staged) (void)hipFree(q);
  };
  bool bad = false;
  // a host array on the device: its contents when `copy` (inputs; outputs too — pixels outside every view keep the caller's)
  auto stage = [&](const void* host, size_t bytes) -> void* {
    if (!host || d->device_ptrs) return const_cast<void*>(host);
    void* q = nullptr;
    if (hipMalloc(&q, bytes) != hipSuccess) {
      bad = true;
      return nullptr;
    }
    staged.push_back(q);
    if (hipMemcpyAsync(q, host, bytes, hipMemcpyHostToDevice, st) != hipSuccess) bad = true;
    return q;
  };
  sthip::DenoiseParams p{};
  p.width = d->width;
  p.height = d->height;
  p.view_count = d->view_count;
  p.instance_count = d->instance_count;
  p.history_limit = d->history_limit;
  p.variance_boost_length = d->variance_boost_length;
  p.sigma_luminance_boost = d->sigma_luminance_boost;
  if (d->view_count <= sthip::DENOISE_INLINE_VIEWS) {  // gViews is a host array in either form
    p.views = nullptr;
    memcpy(p.inline_views, d->gViews, (size_t)d->view_count * sizeof(sthip_ViewData));
  } else {
    void* q = nullptr;
    if (hipMalloc(&q, (size_t)d->view_count * sizeof(sthip_ViewData)) != hipSuccess)
      bad = true;
    else {
      staged.push_back(q);
      if (hipMemcpyAsync(q, d->gViews, (size_t)d->view_count * sizeof(sthip_ViewData), hipMemcpyHostToDevice, st) != hipSuccess) bad = true;
    }
    p.views = (const sthip_ViewData*)q;
  }
  p.visibility = (const sthip_VisibilityInfo*)stage(d->gVisibility, n * sizeof(sthip_VisibilityInfo));
  p.depth = (const sthip_DepthInfo*)stage(d->gDepth, n * sizeof(sthip_DepthInfo));
  p.instance_index_map = (const uint32_t*)stage(d->gInstanceIndexMap, (size_t)d->instance_count * 4);
  p.accum_color = stage(d->gAccumColor, n * cb);
  p.accum_moments = stage(d->gAccumMoments, n * 8);
  p.filter[0] = stage(d->gFilterImages[0], n * cb);
  p.filter[1] = stage(d->gFilterImages[1], n * cb);
  p.guide = ctx->denoise_guide.p;
  if (bad) {
    (void)hipStreamSynchronize(st);
    release();
    return fail(ctx, STHIP_ERR_HIP, "sthip_denoise_filter: staging the host images on the device failed");
  }
  hipEvent_t ev[20] = {};
  bool ran[10] = {};
  hipError_t e = hipSuccess;
  if (d->pass_ms)
    for (int k = 0; k < 20 && e == hipSuccess; k++) e = hipEventCreate(&ev[k]);
  std::string err;
  const bool ok = e == hipSuccess && sthip::denoise_launch(p, d->iterations, d->filter_type, d->history_tap, ctx->half_color, ctx->denoise_block, st,
                                                           d->pass_ms ? reinterpret_cast<void* const*>(ev) : nullptr, ran, err);
  if (ok && !d->device_ptrs) {
    e = hipMemcpyAsync(d->gFilterImages[0], p.filter[0], n * cb, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d->gFilterImages[1], p.filter[1], n * cb, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && tapped) e = hipMemcpyAsync(d->gAccumColor, p.accum_color, n * cb, hipMemcpyDeviceToHost, st);
  }
  // staged copies must outlive the kernels, and the timings need them finished; the device form with inline views only enqueues
  const hipError_t es = (staged.empty() && !d->pass_ms) ? hipSuccess : hipStreamSynchronize(st);
  if (d->pass_ms) {
    for (int k = 0; k < 10; k++) {
      d->pass_ms[k] = 0;
      if (ok && e == hipSuccess && es == hipSuccess && ran[k]) (void)hipEventElapsedTime(&d->pass_ms[k], ev[2 * k], ev[2 * k + 1]);
    }
    for (int k = 0; k < 20; k++)
      if (ev[k]) (void)hipEventDestroy(ev[k]);
  }
  release();
  if (!ok && e == hipSuccess) return fail(ctx, STHIP_ERR_HIP, "sthip_denoise_filter: " + err);
  if (e != hipSuccess || es != hipSuccess) return fail(ctx, STHIP_ERR_HIP, std::string("sthip_denoise_filter: ") + hipGetErrorString(e != hipSuccess ? e : es));
  return STHIP_OK;
}

int sthip_convert_material(sthip_ctx* ctx, const sthip_convert_material_desc* d) {
  if (!ctx || !d) return STHIP_ERR_INVALID_ARGUMENT;
  auto refuse = [&](const char* field, const char* why) { return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, std::string("sthip_convert_material: ") + field + " " + why); };
  if (d->kind >= STHIP_CONVERT_KIND_COUNT) return refuse("kind", "must be below 4 (STHIP_CONVERT_*)");
  if (!d->width) return refuse("width", "is 0");
  if (!d->height) return refuse("height", "is 0");
  if ((uint64_t)d->width * d->height > (1ull << 30)) return refuse("width x height", "is too large (more than 2^30 texels)");
  if (d->output_format > 1) return refuse("output_format", "is no sthip_image_format");
  const bool material = d->kind == STHIP_CONVERT_GLTF_PBR || d->kind == STHIP_CONVERT_DIFFUSE_SPECULAR;
  const bool with_roughness = d->kind == STHIP_CONVERT_DIFFUSE_SPECULAR;
  const size_t n = (size_t)d->width * d->height, out4 = d->output_format ? 4 : 16, out1 = d->output_format ? 1 : 4;
  struct Image {  // one image of the descriptor: its bytes and what a device pointer must be aligned to
    const char* name;
    const void* p;
    size_t bytes, align;
    bool source;
  };
  std::vector<Image> images;
  int i_diffuse = -1, i_specular = -1, i_transmittance = -1, i_roughness = -1, i_input = -1, i_out[3] = {-1, -1, -1}, i_mask = -1, i_min = -1, i_rw = -1;
  auto add = [&](const char* name, const void* p, size_t texel, size_t align, bool source) {
    images.push_back({name, p, texel ? n * texel : 4, align, source});
    return (int)images.size() - 1;
  };
  // a source: format 0 / 1 is the library's own form of `channels` channels, from 16 up a sthip_texel_format (texel_decode.h)
  int format_status = STHIP_OK;
  auto format_ok = [&](const char* field, uint32_t format) {
    if (format <= 1 || (sthip::texel_format_built(format))) return true;
    if (sthip::texel_format_named_unsupported(format))
      format_status = fail(ctx, STHIP_ERR_UNSUPPORTED, std::string("sthip_convert_material: ") + field + " " + std::to_string(format) + " (" + sthip::texel_unsupported_name(format) + ") has no meaning on a material path and is not built");
    else
      format_status = refuse(field, "is no sthip_image_format");
    return false;
  };
  auto add_source = [&](const char* name, const void* p, uint32_t format, size_t channels) {
    if (format <= 1) return add(name, p, format ? channels : 4 * channels, format ? channels : 4 * channels, true);
    images.push_back({name, p, (size_t)sthip::texel_image_bytes(format, d->width, d->height), sthip::texel_alignment(format), true});
    return (int)images.size() - 1;
  };
  if (material) {
    if (!d->gDiffuse && !d->gSpecular && !d->gTransmittance && !(with_roughness && d->gRoughness))
      return refuse(with_roughness ? "gDiffuse / gSpecular / gTransmittance / gRoughness" : "gDiffuse / gSpecular / gTransmittance", "are all NULL: no source");
    if (d->gDiffuse && !format_ok("diffuse_format", d->diffuse_format)) return format_status;
    if (d->gSpecular && !format_ok("specular_format", d->specular_format)) return format_status;
    if (d->gTransmittance && !format_ok("transmittance_format", d->transmittance_format)) return format_status;
    if (with_roughness && d->gRoughness && !format_ok("roughness_format", d->roughness_format)) return format_status;
    if (!d->gOutput[0]) return refuse("gOutput[0]", "is NULL");
    if (!d->gOutput[1]) return refuse("gOutput[1]", "is NULL");
    if (!d->gOutput[2]) return refuse("gOutput[2]", "is NULL");
    if (!d->gOutputMinAlpha) return refuse("gOutputMinAlpha", "is NULL");
    if (d->gDiffuse && !d->gOutputAlphaMask) return refuse("gOutputAlphaMask", "is NULL although gDiffuse is given");
    if (d->gDiffuse) i_diffuse = add_source("gDiffuse", d->gDiffuse, d->diffuse_format, 4);
    if (d->gSpecular) i_specular = add_source("gSpecular", d->gSpecular, d->specular_format, 4);
    if (d->gTransmittance) i_transmittance = add_source("gTransmittance", d->gTransmittance, d->transmittance_format, 4);
    if (with_roughness && d->gRoughness) i_roughness = add_source("gRoughness", d->gRoughness, d->roughness_format, 1);
    i_out[0] = add("gOutput[0]", d->gOutput[0], out4, out4, false);
    i_out[1] = add("gOutput[1]", d->gOutput[1], out4, out4, false);
    i_out[2] = add("gOutput[2]", d->gOutput[2], out4, out4, false);
    if (d->gDiffuse) i_mask = add("gOutputAlphaMask", d->gOutputAlphaMask, out1, out1, false);
    i_min = add("gOutputMinAlpha", d->gOutputMinAlpha, 0, 4, false);  // (one word, whatever the extent)
  } else {
    if (!d->gInput) return refuse("gInput", "is NULL");
    if (!d->gRoughnessRW) return refuse("gRoughnessRW", "is NULL");
    if (!format_ok("input_format", d->input_format)) return format_status;
    i_input = add_source("gInput", d->gInput, d->input_format, 1);
    i_rw = add("gRoughnessRW", d->gRoughnessRW, out1, out1, false);
  }
  if (d->device_ptrs)
    for (const Image& im : images)
      if ((uintptr_t)im.p & (im.align - 1)) return refuse(im.name, "is not naturally aligned");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  // host form: one device buffer per image (DevBuf: freed on return; poisoned under STHIP_POISON_ALLOC), sources copied up
  std::vector<DevBuf<uint8_t>> staged(d->device_ptrs ? 0 : images.size());
  std::vector<void*> dev(images.size());
  for (size_t k = 0; k < images.size(); k++) {
    const size_t bytes = images[k].bytes;
    if (d->device_ptrs) {
      dev[k] = const_cast<void*>(images[k].p);
      continue;
    }
    HIP_TRY(ctx, staged[k].ensure(bytes));
    dev[k] = staged[k].p;
    if (images[k].source) HIP_TRY(ctx, hipMemcpyAsync(dev[k], images[k].p, bytes, hipMemcpyHostToDevice, st));
  }
  auto device_of = [&](int k) -> void* { return k < 0 ? nullptr : dev[k]; };
  sthip::MaterialConvertParams p{};
  p.kind = d->kind;
  p.texels = n;
  p.width = d->width, p.height = d->height;
  p.output_format = d->output_format;
  p.diffuse = device_of(i_diffuse);
  p.specular = device_of(i_specular);
  p.transmittance = device_of(i_transmittance);
  p.roughness = device_of(i_roughness);
  p.input = device_of(i_input);
  p.diffuse_format = d->diffuse_format, p.specular_format = d->specular_format, p.transmittance_format = d->transmittance_format, p.roughness_format = d->roughness_format;
  p.input_format = d->input_format;
  for (int k = 0; k < 3; k++) p.out[k] = device_of(i_out[k]);
  p.alpha_mask = device_of(i_mask);
  p.min_alpha = (uint32_t*)device_of(i_min);
  p.roughness_rw = device_of(i_rw);
  std::string err;
  const bool ok = sthip::material_convert_launch(p, st, err);
  hipError_t e = hipSuccess;
  if (!d->device_ptrs) {  // the staged buffers must outlive the kernel: always synchronise
    for (size_t k = 0; ok && e == hipSuccess && k < images.size(); k++)
      if (!images[k].source) e = hipMemcpyAsync(const_cast<void*>(images[k].p), dev[k], images[k].bytes, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
  }
  if (!ok) return fail(ctx, STHIP_ERR_HIP, "sthip_convert_material: " + err);
  if (e != hipSuccess) return fail(ctx, STHIP_ERR_HIP, std::string("sthip_convert_material: ") + hipGetErrorString(e));
  return STHIP_OK;
}

// A source image in an asset's own texel format to one of the library's four forms (texel_decode.hip).
int sthip_decode_texels(sthip_ctx* ctx, const sthip_decode_texels_desc* d) {
  if (!ctx || !d) return STHIP_ERR_INVALID_ARGUMENT;
  auto refuse = [&](const char* field, const char* why) { return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, std::string("sthip_decode_texels: ") + field + " " + why); };
  if (!d->width) return refuse("width", "is 0");
  if (!d->height) return refuse("height", "is 0");
  if ((uint64_t)d->width * d->height > (1ull << 30)) return refuse("width x height", "is too large (more than 2^30 texels)");
  if (sthip::texel_format_named_unsupported(d->src_format))
    return fail(ctx, STHIP_ERR_UNSUPPORTED, std::string("sthip_decode_texels: src_format ") + std::to_string(d->src_format) + " (" + sthip::texel_unsupported_name(d->src_format) + ") has no meaning on a material path and is not built");
  if (!sthip::texel_format_built(d->src_format)) return refuse("src_format", "is no sthip_texel_format");
  if (d->dst_format > 1) return refuse("dst_format", "is no sthip_image_format");
  if (d->dst_channels != 1 && d->dst_channels != 4) return refuse("dst_channels", "must be 1 or 4");
  if (d->dst_channels == 1 && d->channel > 3) return refuse("channel", "is above 3");
  if (!d->src) return refuse("src", "is NULL");
  if (!d->dst) return refuse("dst", "is NULL");
  const uint32_t f = sthip::texel_canonical(d->src_format);
  const size_t n = (size_t)d->width * d->height, dst_texel = (d->dst_channels == 4 ? 4 : 1) * (d->dst_format ? 1 : 4);
  const size_t src_bytes = (size_t)sthip::texel_image_bytes(f, d->width, d->height), dst_bytes = n * dst_texel;
  if (d->device_ptrs) {
    if ((uintptr_t)d->src & (sthip::texel_alignment(f) - 1)) return refuse("src", "is not naturally aligned");
    if ((uintptr_t)d->dst & (dst_texel - 1)) return refuse("dst", "is not naturally aligned");
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf<uint8_t> staged_src, staged_dst;  // host form only (freed on return; poisoned under STHIP_POISON_ALLOC)
  sthip::TexelDecodeParams p{};
  p.format = f;
  p.width = d->width, p.height = d->height;
  p.dst8 = d->dst_format, p.dst_one = d->dst_channels == 1, p.channel = d->channel;
  p.src = d->src, p.dst = d->dst;
  if (!d->device_ptrs) {
    HIP_TRY(ctx, staged_src.ensure(src_bytes));
    HIP_TRY(ctx, staged_dst.ensure(dst_bytes));
    HIP_TRY(ctx, hipMemcpyAsync(staged_src.p, d->src, src_bytes, hipMemcpyHostToDevice, st));
    p.src = staged_src.p, p.dst = staged_dst.p;
  }
  std::string err;
  const bool ok = sthip::texel_decode_launch(p, st, err);
  hipError_t e = hipSuccess;
  if (!d->device_ptrs) {  // the staged buffers must outlive the kernel: always synchronise
    if (ok) e = hipMemcpyAsync(d->dst, staged_dst.p, dst_bytes, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
  }
  if (!ok) return fail(ctx, STHIP_ERR_HIP, "sthip_decode_texels: " + err);
  if (e != hipSuccess) return fail(ctx, STHIP_ERR_HIP, std::string("sthip_decode_texels: ") + hipGetErrorString(e));
  return STHIP_OK;
}

// ---- beside the path: a NanoVDB density grid from a dense box (volume_build.hip) ----
// The checks of a dense description, the scan with its read-back and every refusal the values decide; then the header and
// `info`. Nothing of the caller's is written before the last refusal. Shared with sthip_scene_set_volume (api.hip).
int dense_volume_scan(sthip_ctx* ctx, const char* call, const sthip_dense_volume_desc* d, DevBuf<float>& staged, sthip::VolumeBuildInput& in, sthip::VolumeBuildCounts& c, sthip::VolumeHeader& header,
                      sthip_volume_info* info, float& scan_ms) {
  auto refuse = [&](const char* field, const char* why) { return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, std::string(call) + ": " + field + " " + why); };
  if (!d) return refuse("desc", "is NULL");
  if (d->struct_size != sizeof(sthip_dense_volume_desc)) return refuse("struct_size", "is not sizeof(sthip_dense_volume_desc)");
  if (!d->dense) return refuse("dense", "is NULL");
  if (d->dense_is_device && ((uintptr_t)d->dense & 3u)) return refuse("dense", "is not 4-byte aligned");
  for (int a = 0; a < 3; a++) {
    if (!d->dims[a]) return refuse("dims", "has a zero extent");
    if ((int64_t)d->origin[a] + (int64_t)d->dims[a] - 1 > (int64_t)INT32_MAX) return refuse("origin + dims", "leaves int32");
    if (!std::isfinite(d->translation[a])) return refuse("translation", "is not finite");
  }
  if (!(d->voxel_size > 0.0) || !std::isfinite(d->voxel_size)) return refuse("voxel_size", "must be finite and positive");
  if (d->name && strlen(d->name) > 255) return refuse("name", "has more than 255 bytes");
  in = sthip::VolumeBuildInput{};
  in.dense = d->dense;
  for (int a = 0; a < 3; a++) in.dims[a] = d->dims[a], in.origin[a] = d->origin[a];
  {
    sthip::VbLattice lattice;
    if (!sthip::vb_lattice(in, lattice)) return refuse("dims", "touch more than 2^24 bricks of 8^3 voxels");
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (!ctx->volume_build) ctx->volume_build = sthip::device_volume_build_create();
  const uint64_t voxels = (uint64_t)d->dims[0] * d->dims[1] * d->dims[2];  // (at most 2^33: the brick limit above)
  if (!d->dense_is_device) {  // the host form: the dense box copied up (the caller's buffer, freed when it returns)
    HIP_TRY(ctx, staged.ensure(voxels));
    HIP_TRY(ctx, hipMemcpyAsync(staged.p, d->dense, voxels * sizeof(float), hipMemcpyHostToDevice, st));
    in.dense = staged.p;
  }
  std::string err;
  if (!sthip::volume_build_scan(ctx->volume_build, in, st, c, scan_ms, err)) {
    (void)hipStreamSynchronize(st);  // (the staged copy must not outlive its buffer)
    return fail(ctx, STHIP_ERR_HIP, std::string(call) + ": " + err);
  }
  // ---- every refusal the values decide ----
  if (c.nonfinite) return refuse("dense", "holds a NaN or an infinite value");
  if (!c.active) return refuse("dense", "has no active voxel (every value is 0)");
  if (c.uppers > sthip::NVDB_MAX_TILES) return refuse("dense", "needs more than 65536 root tiles");
  const sthip::VolumeLayout lay = sthip::volume_layout(c);
  if (lay.total > sthip::NVDB_MAX_BYTES) return refuse("dense", "gives a grid of more than 0xFFFFFFF0 bytes");
  memset(info, 0, sizeof(*info));
  sthip::volume_header(c, d->voxel_size, d->translation, d->name, header, info->world_bbox);
  info->bytes = lay.total;
  for (int a = 0; a < 3; a++) info->bbox_min[a] = c.bbox_min[a], info->bbox_max[a] = c.bbox_max[a];
  info->min = c.min, info->max = c.max;
  info->active_voxels = c.active;
  info->leaf_count = c.leaves, info->lower_count = c.lowers, info->upper_count = c.uppers, info->root_tiles = c.uppers;
  info->device_ms = scan_ms;
  return STHIP_OK;
}

int sthip_build_volume(sthip_ctx* ctx, const sthip_dense_volume_desc* d, void* out, uint64_t capacity, int out_is_device, sthip_volume_info* info) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  const auto t0 = std::chrono::steady_clock::now();
  auto wall = [&]() { return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
  if (!info) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_build_volume: info is NULL");
  if (out && out_is_device && ((uintptr_t)out & 31u)) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_build_volume: out is a device pointer that is not 32-byte aligned");
  DevBuf<float> staged;
  sthip::VolumeBuildInput in{};
  sthip::VolumeBuildCounts c{};
  sthip::VolumeHeader header;
  float scan_ms = 0, emit_ms = 0;
  if (const int rc = dense_volume_scan(ctx, "sthip_build_volume", d, staged, in, c, header, info, scan_ms); rc != STHIP_OK) return rc;
  const uint64_t total = info->bytes;
  info->call_ms = wall();
  if (!out || capacity < total) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_build_volume: the grid has " + std::to_string(total) + " bytes, capacity is " + std::to_string(capacity));
  // ---- emit ----
  std::string err;
  void* target = out;
  if (!out_is_device) {
    target = sthip::volume_build_staging(ctx->volume_build, total, err);
    if (!target) return fail(ctx, STHIP_ERR_HIP, "sthip_build_volume: " + err);
  }
  if (!sthip::volume_build_emit(ctx->volume_build, in, c, header, target, ctx->stream, emit_ms, err)) {
    (void)hipStreamSynchronize(ctx->stream);
    return fail(ctx, STHIP_ERR_HIP, "sthip_build_volume: " + err);
  }
  if (!out_is_device) HIP_TRY(ctx, hipMemcpy(out, target, total, hipMemcpyDeviceToHost));
  info->device_ms = scan_ms + emit_ms;
  info->call_ms = wall();
  return STHIP_OK;
}

// C: the colour images' element, float4 (RGBA32F) or Half4 ("half_color_precision")
template <typename C>
static int tonemap_images(sthip_ctx* ctx, const sthip_tonemap_desc* d);
template <typename C>
static int compare_images(sthip_ctx* ctx, const float* image1, const float* image2, uint32_t width, uint32_t height, uint32_t metric, uint32_t quantization, uint32_t device_ptrs,
                          uint32_t* sum_out, uint32_t* overflow_out);
int sthip_tonemap(sthip_ctx* ctx, const sthip_tonemap_desc* d) {
  if (!ctx || !d) return STHIP_ERR_INVALID_ARGUMENT;
  if (!d->gInput || !d->gOutput || d->width == 0 || d->height == 0) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_tonemap: gInput, gOutput and a non-empty extent are required");
  if (d->mode >= eTonemapModeCount) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_tonemap: unknown mode " + std::to_string(d->mode));
  if (d->modulate_albedo && !d->gAlbedo) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_tonemap: gModulateAlbedo needs gAlbedo");
  if ((uint64_t)d->width * d->height > 0xFFFFFFFFull) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_tonemap: extent too large");
  return ctx->half_color ? tonemap_images<Half4>(ctx, d) : tonemap_images<float4>(ctx, d);
}
template <typename C>
static int tonemap_images(sthip_ctx* ctx, const sthip_tonemap_desc* d) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint32_t n = d->width * d->height;
  const C *in = reinterpret_cast<const C*>(d->gInput), *alb = reinterpret_cast<const C*>(d->gAlbedo);
  C* out = reinterpret_cast<C*>(d->gOutput);
  DevBuf<C> bin, balb, bout;
  if (!d->device_ptrs) {
    HIP_TRY(ctx, bin.ensure(n));
    HIP_TRY(ctx, bout.ensure(n));
    HIP_TRY(ctx, hipMemcpyAsync(bin.p, d->gInput, (size_t)n * sizeof(C), hipMemcpyHostToDevice, st));
    in = bin.p;
    out = bout.p;
    if (d->modulate_albedo) {
      HIP_TRY(ctx, balb.ensure(n));
      HIP_TRY(ctx, hipMemcpyAsync(balb.p, d->gAlbedo, (size_t)n * sizeof(C), hipMemcpyHostToDevice, st));
      alb = balb.p;
    }
  }
  HIP_TRY(ctx, ctx->post_scratch.ensure(16));  // 4 quantised maxima, then the 6 floats of the exposure state
  HIP_TRY(ctx, hipMemsetAsync(ctx->post_scratch.p, 0, 16, st));
  TonemapState prev;
  for (int k = 0; k < 6; k++) prev.v[k] = d->exposure_state ? d->exposure_state[k] : 0.0f;
  float* state_out = d->exposure_state ? reinterpret_cast<float*>(ctx->post_scratch.p + 4) : nullptr;
  const uint32_t grid = (uint32_t)std::min<size_t>(((size_t)n + 255) / 256, (size_t)ctx->cu_count * 16);
  hipLaunchKernelGGL(k_tonemap_reduce_max<C>, dim3(grid), dim3(256), 0, st, in, alb, n, d->modulate_albedo, ctx->post_scratch.p);
  hipLaunchKernelGGL(k_tonemap<C>, dim3(grid), dim3(256), 0, st, in, alb, out, n, d->mode, d->modulate_albedo, d->gamma_correction, d->exposure, ctx->post_scratch.p,
                     d->exposure_state ? d->exposure_alpha : 0.0f, prev, state_out);
  HIP_TRY(ctx, hipGetLastError());
  if (!d->device_ptrs) HIP_TRY(ctx, hipMemcpyAsync(d->gOutput, bout.p, (size_t)n * sizeof(C), hipMemcpyDeviceToHost, st));
  if (d->out_max) {
    uint32_t m[4];
    HIP_TRY(ctx, hipMemcpyAsync(m, ctx->post_scratch.p, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (int k = 0; k < 4; k++) d->out_max[k] = (float)m[k] / TONEMAP_MAX_QUANTIZATION;
  } else if (!d->device_ptrs) {
    HIP_TRY(ctx, hipStreamSynchronize(st));
  }
  if (d->exposure_state) {  // the state goes back to the caller: this form of the call synchronises
    HIP_TRY(ctx, hipMemcpyAsync(d->exposure_state, state_out, 24, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
  }
  return STHIP_OK;
}

int sthip_image_compare(sthip_ctx* ctx, const float* image1, const float* image2, uint32_t width, uint32_t height, uint32_t metric, uint32_t quantization, uint32_t device_ptrs,
                        uint32_t* sum_out, uint32_t* overflow_out) {
  if (!ctx) return STHIP_ERR_INVALID_ARGUMENT;
  if (!image1 || !image2 || !sum_out || width == 0 || height == 0) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_image_compare: two images, sum_out and a non-empty extent are required");
  if (metric > 2) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_image_compare: unknown metric " + std::to_string(metric));
  if ((uint64_t)width * height * 3 > 0xFFFFFFFFull) return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_image_compare: extent too large");
  return ctx->half_color ? compare_images<Half4>(ctx, image1, image2, width, height, metric, quantization, device_ptrs, sum_out, overflow_out)
                         : compare_images<float4>(ctx, image1, image2, width, height, metric, quantization, device_ptrs, sum_out, overflow_out);
}
template <typename C>
static int compare_images(sthip_ctx* ctx, const float* image1, const float* image2, uint32_t width, uint32_t height, uint32_t metric, uint32_t quantization, uint32_t device_ptrs,
                          uint32_t* sum_out, uint32_t* overflow_out) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint32_t n = width * height;
  const C *a = reinterpret_cast<const C*>(image1), *b = reinterpret_cast<const C*>(image2);
  DevBuf<C> ba, bb;
  if (!device_ptrs) {
    HIP_TRY(ctx, ba.ensure(n));
    HIP_TRY(ctx, bb.ensure(n));
    HIP_TRY(ctx, hipMemcpyAsync(ba.p, image1, (size_t)n * sizeof(C), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(bb.p, image2, (size_t)n * sizeof(C), hipMemcpyHostToDevice, st));
    a = ba.p;
    b = bb.p;
  }
  HIP_TRY(ctx, ctx->post_scratch.ensure(4));
  HIP_TRY(ctx, hipMemsetAsync(ctx->post_scratch.p, 0, 16, st));
  hipLaunchKernelGGL(k_image_compare<C>, dim3((n + 63) / 64), dim3(64), 0, st, a, b, n, metric, quantization, ctx->post_scratch.p);
  HIP_TRY(ctx, hipGetLastError());
  uint32_t r[2];
  HIP_TRY(ctx, hipMemcpyAsync(r, ctx->post_scratch.p, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  *sum_out = r[0];
  if (overflow_out) *overflow_out = r[1];
  return STHIP_OK;
}

// ---- measured ceilings for the roofline (ceilings.h) ----
int sthip_measure_ceiling(sthip_ctx* ctx, uint32_t kind, double* gbytes_per_s) {
  if (!ctx || !gbytes_per_s) return STHIP_ERR_INVALID_ARGUMENT;
  *gbytes_per_s = 0.0;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint32_t blocks = (uint32_t)ctx->cu_count * 8u;  // 2048 threads per CU: every wave slot
  float best_ms = 0.0f;
  double bytes = 0.0;
  if (kind == STHIP_CEILING_TRIAD) {
    const size_t n = (size_t)32 << 20;  // 3 arrays of 512 MiB: far beyond the 256 MiB Infinity Cache
    DevBuf<float4> a, b, c;
    HIP_TRY(ctx, a.ensure(n));
    HIP_TRY(ctx, b.ensure(n));
    HIP_TRY(ctx, c.ensure(n));
    HIP_TRY(ctx, hipMemsetAsync(a.p, 0, n * 16, st));
    HIP_TRY(ctx, hipMemsetAsync(b.p, 0, n * 16, st));
    bytes = 3.0 * 16.0 * (double)n;
    for (int rep = 0; rep < 4; rep++) {
      HIP_TRY(ctx, hipEventRecord(ctx->ev[0], st));
      hipLaunchKernelGGL(k_ceiling_triad, dim3(blocks), dim3(256), 0, st, a.p, b.p, c.p, 0.5f, n);
      HIP_TRY(ctx, hipEventRecord(ctx->ev[1], st));
      HIP_TRY(ctx, hipEventSynchronize(ctx->ev[1]));
      float ms = 0;
      HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
      if (rep > 0 && (best_ms == 0.0f || ms < best_ms)) best_ms = ms;
    }
  } else if (kind == STHIP_CEILING_NODE_GATHER_TABLE || kind == STHIP_CEILING_NODE_GATHER_L2 || kind == STHIP_CEILING_NODE_GATHER_L1) {
    if (!ctx->has_scene || !ctx->bvh_nodes) return fail(ctx, STHIP_ERR_NO_SCENE, "sthip_measure_ceiling: the node-gather ceilings read the resident acceleration structure: upload a scene first");
    // the nodes k_trace walks: the 48-byte binary ones (3 loads), the 64-byte 4-wide ones (4 loads) or the 80-byte 8-wide ones (5 loads)
    const bool wide8 = ctx->bvh.wide8_nodes != nullptr, wide = !wide8 && ctx->bvh.wide_nodes != nullptr;
    const uint32_t nb = wide8 ? (uint32_t)sizeof(Wide8Node) : wide ? (uint32_t)sizeof(WideNode) : BVH_NODE_BYTES;
    uint32_t count = (uint32_t)std::min<uint64_t>(wide8 ? ctx->wide8_node_count : wide ? ctx->wide_node_count : ctx->bvh_nodes, 0xFFFFFFFFull);
    if (kind == STHIP_CEILING_NODE_GATHER_L2) count = std::min<uint32_t>(count, (2u << 20) / nb);
    if (kind == STHIP_CEILING_NODE_GATHER_L1) count = std::min<uint32_t>(count, (16u << 10) / nb);
    const uint32_t iterations = 64;
    DevBuf<float> sink;
    HIP_TRY(ctx, sink.ensure((size_t)blocks * 256));
    bytes = (double)(wide8 ? sizeof(Wide8Node) : wide ? sizeof(WideNode) : sizeof(BvhNodePacked)) * (double)blocks * 256.0 * iterations * CEIL_UNROLL;
    for (int rep = 0; rep < 4; rep++) {
      HIP_TRY(ctx, hipEventRecord(ctx->ev[0], st));
      if (wide8)
        hipLaunchKernelGGL(k_ceiling_node_gather<5>, dim3(blocks), dim3(256), 0, st, reinterpret_cast<const float4*>(ctx->wide8_nodes.p), count, nb, iterations, sink.p);
      else if (wide)
        hipLaunchKernelGGL(k_ceiling_node_gather<4>, dim3(blocks), dim3(256), 0, st, reinterpret_cast<const float4*>(ctx->wide_nodes.p), count, nb, iterations, sink.p);
      else
        hipLaunchKernelGGL(k_ceiling_node_gather<3>, dim3(blocks), dim3(256), 0, st, reinterpret_cast<const float4*>(ctx->nodes.p), count, nb, iterations, sink.p);
      HIP_TRY(ctx, hipEventRecord(ctx->ev[1], st));
      HIP_TRY(ctx, hipEventSynchronize(ctx->ev[1]));
      float ms = 0;
      HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
      if (rep > 0 && (best_ms == 0.0f || ms < best_ms)) best_ms = ms;
    }
  } else {
    return fail(ctx, STHIP_ERR_INVALID_ARGUMENT, "sthip_measure_ceiling: unknown kind");
  }
  HIP_TRY(ctx, hipGetLastError());
  if (best_ms > 0.0f) *gbytes_per_s = bytes / ((double)best_ms * 1e-3) / 1e9;
  return STHIP_OK;
}

