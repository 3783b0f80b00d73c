// async_host.cpp — the pipelined host outputs (include/sthip.h: sthip_render_async) from C++.
//   async_host frames <scene.bin> <out.bin> <seeds> sync|async
//       three frames of a sliding camera through BDPT::render (sync) or BDPT::submit / BDPT::finish with two frames in
//       flight (async); per frame writes prev_result()'s radiance, tone-mapped result, prev-uv and ray counts
//   async_host gate <scene.bin>
//       completion happens at the wait, not before and not at submit: the render stream is held by a host function (the
//       gate) while sthip_render_async is called. While the gate is closed the call must have returned,
//       sthip_outputs_ready must be 0 and the pinned buffers must still hold their 0xFF fill; after the gate opens,
//       sthip_wait_outputs delivers the bytes of the synchronous call. A watchdog opens the gate after 20 s whatever
//       happens, so that a submit call that wrongly synchronises is a clean failure and not a stuck process. A blocked
//       host function is an idle stream: nothing here faults the device.
#include <hip/hip_runtime.h>

#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <fstream>
#include <mutex>
#include <thread>

#include "../../stratum_amd/host/stratum_hip.hpp"
#include "scene_reader.hpp"

using namespace stm;

namespace {
struct Gate {
  std::mutex m;
  std::condition_variable cv;
  bool open = false;
  bool opened_by_watchdog = false;
  bool done = false;  // the test is over: the watchdog may leave
};

void gate_fn(void* user) {  // runs on a runtime thread when the stream reaches it; holds the stream until the gate opens
  Gate* g = static_cast<Gate*>(user);
  std::unique_lock<std::mutex> lock(g->m);
  g->cv.wait(lock, [g] { return g->open; });
}

struct RawBDPT : BDPT {  // the context and the resolved flags, for calls through the C ABI itself
  using BDPT::BDPT;
  sthip_ctx* ctx() { return mCtx; }
  uint32_t flags() const { return sampling_flags(); }
};

struct Images {
  uint8_t *radiance, *albedo, *visibility, *depth, *prev_uv;
  uint64_t* ray_count;
  size_t n;
  size_t bytes(int k) const { return n * (k < 2 ? 16 : k == 3 ? 16 : 8); }
  uint8_t* image(int k) const { return k == 0 ? radiance : k == 1 ? albedo : k == 2 ? visibility : k == 3 ? depth : prev_uv; }
  sthip_outputs outputs() const {
    sthip_outputs o{};
    o.gRadiance = reinterpret_cast<float*>(radiance);
    o.gAlbedo = reinterpret_cast<float*>(albedo);
    o.gVisibility = reinterpret_cast<VisibilityInfo*>(visibility);
    o.gDepth = reinterpret_cast<DepthInfo*>(depth);
    o.gPrevUVs = reinterpret_cast<float*>(prev_uv);
    o.gRayCount = ray_count;
    return o;
  }
};

#define HIP_OK(expr)                                                        \
  do {                                                                      \
    hipError_t e_ = (expr);                                                 \
    if (e_ != hipSuccess) {                                                 \
      std::printf("FAIL: %s: %s\n", #expr, hipGetErrorString(e_));          \
      return 1;                                                             \
    }                                                                       \
  } while (0)

template <typename T>
void put(std::ofstream& out, const std::vector<T>& v) {
  out.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

int run_gate(RawBDPT& r, const LoadedScene& L) {
  sthip_ctx* ctx = r.ctx();
  const size_t n = (size_t)L.W * L.H;
  BDPT::FrameSetup fs;
  r.prepare_frame(L.W, L.H, {{L.view, L.view_xf}}, fs);
  // the synchronous frame, into ordinary memory
  std::vector<uint8_t> sync_mem(n * 64);
  uint64_t sync_rays[2] = {0, 0};
  Images ref{sync_mem.data(), sync_mem.data() + 16 * n, sync_mem.data() + 32 * n, sync_mem.data() + 40 * n, sync_mem.data() + 56 * n, sync_rays, n};
  sthip_outputs o = ref.outputs();
  if (sthip_render(ctx, &fs.pc, r.flags(), fs.scene_flags, &fs.f, 7, 1, &o) != STHIP_OK) {
    std::printf("FAIL: sthip_render: %s\n", sthip_last_error(ctx));
    return 1;
  }
  // pinned buffers, filled with 0xFF
  void* block = nullptr;
  if (sthip_host_alloc(ctx, n * 64 + 16, &block) != STHIP_OK) {
    std::printf("FAIL: sthip_host_alloc: %s\n", sthip_last_error(ctx));
    return 1;
  }
  uint8_t* q = static_cast<uint8_t*>(block);
  std::memset(q, 0xFF, n * 64 + 16);
  Images got{q, q + 16 * n, q + 32 * n, q + 40 * n, q + 56 * n, reinterpret_cast<uint64_t*>(q + 64 * n), n};
  // the gate: a host function that holds the render stream
  hipStream_t stream = nullptr;
  HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  if (sthip_set_stream(ctx, stream) != STHIP_OK) {
    std::printf("FAIL: sthip_set_stream\n");
    return 1;
  }
  Gate gate;
  std::thread watchdog([&gate] {
    std::unique_lock<std::mutex> lock(gate.m);
    if (!gate.cv.wait_for(lock, std::chrono::seconds(20), [&gate] { return gate.done || gate.open; })) {
      gate.open = true;
      gate.opened_by_watchdog = true;
      gate.cv.notify_all();
    }
  });
  auto open_gate = [&gate] {
    std::lock_guard<std::mutex> lock(gate.m);
    gate.open = true;
    gate.cv.notify_all();
  };
  auto finish = [&](int rc) {
    {
      std::lock_guard<std::mutex> lock(gate.m);
      gate.open = true;
      gate.done = true;
      gate.cv.notify_all();
    }
    watchdog.join();
    (void)hipStreamSynchronize(stream);
    (void)sthip_set_stream(ctx, nullptr);
    (void)sthip_host_free(ctx, block);
    (void)hipStreamDestroy(stream);
    return rc;
  };
  if (hipLaunchHostFunc(stream, gate_fn, &gate) != hipSuccess) {
    std::printf("FAIL: hipLaunchHostFunc\n");
    return finish(1);
  }
  std::vector<ViewData> views_copy = fs.v;  // the arguments are borrowed for the call only: this array is overwritten once the call has returned
  fs.f.gViews = views_copy.data();
  o = got.outputs();
  uint64_t ticket = 0;
  const int rc = sthip_render_async(ctx, &fs.pc, r.flags(), fs.scene_flags, &fs.f, 7, 1, &o, &ticket);
  bool closed_at_return;
  {
    std::lock_guard<std::mutex> lock(gate.m);
    closed_at_return = !gate.open;
  }
  if (rc != STHIP_OK) {
    std::printf("FAIL: sthip_render_async: %s\n", sthip_last_error(ctx));
    return finish(1);
  }
  if (!closed_at_return) {
    std::printf("FAIL: sthip_render_async returned only after the gate opened (it waited for the stream)\n");
    return finish(1);
  }
  std::memset(views_copy.data(), 0xAB, views_copy.size() * sizeof(ViewData));  // the caller's array is the caller's again
  const int ready = sthip_outputs_ready(ctx, ticket);
  bool untouched = true;
  for (size_t i = 0; i < n * 64 + 16 && untouched; i++) untouched = q[i] == 0xFF;
  bool still_closed;
  {
    std::lock_guard<std::mutex> lock(gate.m);
    still_closed = !gate.open;
  }
  if (!still_closed) {
    std::printf("FAIL: the checks behind the closed gate took until the watchdog opened it\n");
    return finish(1);
  }
  if (ready != 0) {
    std::printf("FAIL: sthip_outputs_ready = %d while the render stream is held\n", ready);
    return finish(1);
  }
  if (!untouched) {
    std::printf("FAIL: the output buffers changed while the render stream is held\n");
    return finish(1);
  }
  open_gate();
  if (sthip_wait_outputs(ctx, ticket) != STHIP_OK) {
    std::printf("FAIL: sthip_wait_outputs: %s\n", sthip_last_error(ctx));
    return finish(1);
  }
  if (sthip_outputs_ready(ctx, ticket) != 1 || sthip_wait_outputs(ctx, ticket) != STHIP_OK) {
    std::printf("FAIL: a finished ticket is not ready / cannot be waited for twice\n");
    return finish(1);
  }
  for (int k = 0; k < 5; k++)
    if (std::memcmp(got.image(k), ref.image(k), ref.bytes(k)) != 0) {
      std::printf("FAIL: image %d differs from the synchronous call's\n", k);
      return finish(1);
    }
  if (got.ray_count[0] != sync_rays[0] || got.ray_count[1] != sync_rays[1] || sync_rays[0] == 0) {
    std::printf("FAIL: gRayCount %llu %llu against %llu %llu\n", (unsigned long long)got.ray_count[0], (unsigned long long)got.ray_count[1], (unsigned long long)sync_rays[0],
                (unsigned long long)sync_rays[1]);
    return finish(1);
  }
  sthip_stats st{};
  if (sthip_get_stats(ctx, &st) != STHIP_OK || st.rays_total != sync_rays[0] || st.rays_path != sync_rays[1]) {
    std::printf("FAIL: sthip_get_stats after the wait does not describe the frame\n");
    return finish(1);
  }
  std::printf("GATE OK %ux%u rays %llu\n", L.W, L.H, (unsigned long long)sync_rays[0]);
  return finish(0);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: async_host frames scene.bin out.bin seeds sync|async | gate scene.bin\n");
    return 2;
  }
  try {
    const std::string mode = argv[1];
    Reader rd(argv[2]);
    NodeGraph graph;
    Node& root = graph.emplace("Instance");
    auto app = root.make_child("Application").make_component<Application>();
    LoadedScene L = load_scene(rd, app.node());
    CommandBuffer cb;
    auto renderer = app.node().make_child("BDPT").make_component<RawBDPT>();
    app->run_frame(cb);  // Scene::update / BDPT::update: the scene is bound
    if (mode == "gate") return run_gate(*renderer, L);
    if (mode == "frames" && argc >= 6) {
      const uint32_t seeds = (uint32_t)std::atoi(argv[4]);
      const bool async = std::string(argv[5]) == "async";
      renderer->tonemap_mode() = STHIP_TONEMAP_ACES;
      renderer->exposure() = 0.5f;
      std::ofstream out(argv[3], std::ios::binary);
      auto views_of = [&](int k) {
        TransformData t = L.view_xf;
        t.m[0][3] += 0.03f * (float)k;
        t.m[1][3] += 0.01f * (float)k;
        return std::vector<std::pair<ViewData, TransformData>>{{L.view, t}};
      };
      auto write_frame = [&] {
        const auto& fr = renderer->prev_result();
        put(out, fr.mRadiance);
        put(out, fr.mTonemapResult);
        put(out, fr.mPrevUVs);
        out.write(reinterpret_cast<const char*>(fr.mRayCount), 16);
        return fr.mRadiance.size() == (size_t)L.W * L.H * 4 && fr.mTonemapResult.size() == fr.mRadiance.size();
      };
      bool ok = true;
      if (async) {  // two frames in flight
        const uint64_t t0 = renderer->submit(cb, L.W, L.H, views_of(0), seeds);
        const uint64_t t1 = renderer->submit(cb, L.W, L.H, views_of(1), seeds);
        renderer->finish(t0);
        ok = write_frame() && ok;
        const uint64_t t2 = renderer->submit(cb, L.W, L.H, views_of(2), seeds);
        renderer->finish(t1);
        ok = write_frame() && ok;
        renderer->finish(t2);
        ok = write_frame() && ok;
      } else {
        for (int k = 0; k < 3; k++) {
          renderer->render(cb, L.W, L.H, views_of(k), seeds);
          ok = write_frame() && ok;
        }
      }
      if (!ok) {
        std::printf("FAIL: a frame's images have the wrong sizes\n");
        return 1;
      }
      std::printf("FRAMES OK %s %ux%u\n", async ? "async" : "sync", L.W, L.H);
      return 0;
    }
    std::fprintf(stderr, "bad arguments\n");
    return 2;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
