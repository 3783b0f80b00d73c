"""Pipelined host outputs (include/sthip.h: sthip_render_async, sthip_outputs_ready, sthip_wait_outputs, sthip_host_alloc,
option "output_ring"): frame i + 1 renders while frame i copies back to host memory on a copy stream of the library's own.

The claim under test is identity: after the wait a frame's five images and gRayCount hold, byte for byte, what the
synchronous sthip_render with the same arguments writes. Both sides are this library, so every comparison is
np.array_equal on the raw bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from stratum_amd import camera, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG_SETS = [(), ("~nee",), ("connecttoviews",), ("connecttolightpaths",), ("neereservoirs", "neereservoirreuse")]  # = test_half_precision.FLAG_SETS
NEW_CALLS = ("sthip_host_alloc", "sthip_host_free", "sthip_render_async", "sthip_outputs_ready", "sthip_wait_outputs")
ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = -1, -4  # sthip_status


def foggy_cornell():
    return scenes.cornell_box(fog=np.load(os.path.join(ROOT, "tests", "golden", "fog_sphere.npz"))["grid"], anisotropy=0.3)


# ---- without a GPU ----
def test_header_documents_the_calls_and_the_option():
    hdr = open(os.path.join(ROOT, "include", "sthip.h")).read()
    for name in NEW_CALLS:
        assert "int %s(" % name in hdr, name
    assert '"output_ring"' in hdr and "1..8" in hdr
    for word in ("borrowed until sthip_wait_outputs", "Pageable", "submission order", "STHIP_ERR_UNSUPPORTED", "device_ptrs must be 0"):
        assert word in hdr, word


def test_loader_declares_the_calls():
    from stratum_amd import _lib

    for name in NEW_CALLS:
        assert name in _lib.EXPORTS, name


def _compile_async_host(exe):
    """The driver, -Wall -Werror against the host headers; links the library, RCCL and the HIP runtime (as test_half_precision's)."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    lib = os.path.join(ROOT, "stratum_amd")
    subprocess.check_call(
        ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "async_host.cpp")]
        + ["-L" + lib, "-lstratum_hip", "-L" + os.path.join(rocm, "lib"), "-lrccl", "-lamdhip64", "-lpthread", "-Wl,-rpath," + lib, "-Wl,-rpath," + os.path.join(rocm, "lib")]
    )
    return exe


@pytest.fixture(scope="module")
def async_host(built, tmp_path_factory):
    return _compile_async_host(str(tmp_path_factory.mktemp("async_host") / "async_host"))


def test_async_host_driver_compiles(async_host):
    assert os.path.exists(async_host)


def test_python_methods_raise_without_a_device_or_scene(built, cornell):
    """As render(): no device -> the constructor raises StratumHipError; with one, a call before update() does."""
    from stratum_amd._lib import StratumHipError
    from stratum_amd.bdpt import BDPT

    for name in ("alloc_host_outputs", "render_async", "wait", "ready"):
        assert callable(getattr(BDPT, name)), name
    _, cam = cornell
    frame = camera.Frame(32, 16, cam["fovy"], cam["eye"], cam["target"])
    with pytest.raises(StratumHipError):
        r = BDPT(device=0)
        try:
            r.render_async(frame, 0, 1)
        finally:
            r.close()


# ---- GPU ----
def _renderer(sc, flags=(), half=False, args=None, ring=None):
    from stratum_amd.bdpt import BDPT

    a = {"bdptFlag": list(flags)}
    a.update(args or {})
    r = BDPT(device=0, args=a)
    r.update(sc)
    if half:
        r.set_half_color_precision(True)
    if ring is not None:
        r.set_option("output_ring", ring)
    return r


def _copy(out):
    return {k: v.copy() for k, v in out.items()}


def _pageable_like(out):
    """Ordinary numpy arrays of the same shapes, filled with bytes no frame holds."""
    res = {}
    for k, v in out.items():
        a = np.empty_like(v)
        a.view(np.uint8)[...] = 0xA5
        res[k] = a
    return res


def _assert_same(got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), (what, k)


def _identity_case(r, frame, seeds, what, packed=False):
    for seed_count in seeds:
        want = _copy(r.render(frame, 3, seed_count, packed_tiles=packed))
        pinned = r.alloc_host_outputs(frame, packed_tiles=packed)
        got = r.wait(r.render_async(frame, 3, seed_count, host_outputs=pinned, packed_tiles=packed))
        assert got["radiance"] is pinned["radiance"]
        _assert_same(got, want, "%s seeds=%d pinned" % (what, seed_count))
        st = r.stats()
        assert st["rays_total"] == int(want["ray_count"][0]) and st["rays_path"] == int(want["ray_count"][1]), what
        pageable = _pageable_like(want)
        got = r.wait(r.render_async(frame, 3, seed_count, host_outputs=pageable, packed_tiles=packed))
        _assert_same(got, want, "%s seeds=%d pageable" % (what, seed_count))


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("flags", FLAG_SETS)
def test_async_equals_sync_flag_sets(built, cornell, flags, half):
    sc, cam = cornell
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    r = _renderer(sc, flags, half=half)
    try:
        _identity_case(r, frame, (1, 3), "flags=%s half=%s" % (flags, half))
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_async_equals_sync_media(built, half):
    sc, cam = foggy_cornell()
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    r = _renderer(sc, half=half)
    try:
        _identity_case(r, frame, (1, 3), "fog half=%s" % half)
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_async_equals_sync_packed_tiles_on_a_shard(built, cornell, half):
    sc, cam = cornell
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    r = _renderer(sc, half=half)
    try:
        for rank in range(2):
            r.set_shard(rank, 2, 16, 8)
            _identity_case(r, frame, (1, 3), "shard %d/2 packed half=%s" % (rank, half), packed=True)
            _identity_case(r, frame, (1,), "shard %d/2 image layout half=%s" % (rank, half), packed=False)
    finally:
        r.close()


def _moving_frames(cam, n, w=96, h=64):
    frames, prev = [], None
    for k in range(n):
        eye = np.array(cam["eye"]) + np.array([0.05, 0.02, 0.0]) * k
        prev = camera.Frame(w, h, cam["fovy"], tuple(eye), cam["target"], prev=prev)
        frames.append(prev)
    return frames


@pytest.mark.gpu
def test_pipeline_of_six_frames(built, cornell):
    """Six frames of a moving camera, ring of 2, six output sets: submitted without a wait in between (the library itself waits
    for the oldest copy when the ring is full), collected in order. Frame k is the synchronous frame k, prev-uv included."""
    sc, cam = cornell
    frames = _moving_frames(cam, 6)
    ref = _renderer(sc)
    try:
        want = [_copy(ref.render(f, k, 1)) for k, f in enumerate(frames)]
    finally:
        ref.close()
    assert not np.array_equal(want[1]["prev_uv"], want[0]["prev_uv"]) and not np.array_equal(want[1]["radiance"], want[2]["radiance"])
    r = _renderer(sc, ring=2)
    try:
        sets = [r.alloc_host_outputs(f) for f in frames]
        tickets = [r.render_async(f, k, 1, host_outputs=sets[k]) for k, f in enumerate(frames)]
        assert tickets == list(range(tickets[0], tickets[0] + 6))
        for k, t in enumerate(tickets):
            got = r.wait(t)
            assert all(r.ready(u) for u in tickets[: k + 1])
            _assert_same(got, want[k], "frame %d" % k)
            assert r.stats()["rays_total"] == int(want[k]["ray_count"][0]), k
    finally:
        r.close()


@pytest.mark.gpu
def test_pipeline_keeps_the_reservoir_chain(built, cornell):
    """neereservoirs + neereservoirreuse with reuse_grids_persist = 1: six async one-seed calls are the chain one synchronous
    six-seed call traces — the running mean (temporal_accumulation.hlsl:118-131) of the six frames, bit for bit, and the same
    rays — because the render work of all frames stays in one stream order."""
    sc, cam = cornell
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    r = _renderer(sc, ("neereservoirs", "neereservoirreuse"), args={"reservoirM": 2}, ring=2)
    try:
        chain = _copy(r.render(frame, 4, 6, aovs=False))
        alone = _copy(r.render(frame, 5, 1, aovs=False))  # a chain of its own
        r.set_option("reuse_grids_persist", 1)
        sets = [r.alloc_host_outputs(frame, aovs=False) for _ in range(6)]
        tickets = [r.render_async(frame, 4 + i, 1, host_outputs=sets[i], aovs=False) for i in range(6)]
        kept = [r.wait(t) for t in tickets]
        assert not np.array_equal(kept[1]["radiance"], alone["radiance"])  # (the second frame did look into the first one's grid)
        acc = kept[0]["radiance"].copy()  # k_resolve's running mean: rgb and, in .w, the samples that counted
        for f in (k["radiance"] for k in kept[1:]):
            nn = acc[..., 3] + f[..., 3]
            with np.errstate(all="ignore"):
                alpha = np.clip(f[..., 3] / nn, np.float32(0), np.float32(1))[..., None]
            live = acc[..., 3] > 0
            rgb = np.where(live[..., None], acc[..., :3] + alpha * (f[..., :3] - acc[..., :3]), f[..., :3])
            acc = np.concatenate([rgb, np.where(live, nn, f[..., 3])[..., None]], -1).astype(np.float32)
        assert np.array_equal(acc.view(np.uint32), chain["radiance"].view(np.uint32))
        assert np.array_equal(sum(k["ray_count"] for k in kept), chain["ray_count"])
    finally:
        r.close()


@pytest.mark.gpu
def test_ring_and_ticket_rules(built, cornell):
    import ctypes as C

    import torch

    from stratum_amd import wire
    from stratum_amd._lib import StratumHipError

    sc, cam = cornell
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    frames = _moving_frames(cam, 3)
    r = _renderer(sc)
    try:
        L, h = r._lib, r._h
        for v in range(1, 9):
            r.set_option("output_ring", v)
        for v in (0, 9, -1):
            with pytest.raises(StratumHipError, match="output_ring"):
                r.set_option("output_ring", v)
        r.set_option("output_ring", 2)
        want = _copy(r.render(frame, 0, 1))
        for t in (0, 1, 77):  # never issued
            assert L.sthip_wait_outputs(h, t) == ERR_INVALID_ARGUMENT and L.sthip_outputs_ready(h, t) == ERR_INVALID_ARGUMENT
        t1 = r.render_async(frame, 0, 1)
        assert t1 == 1
        assert L.sthip_wait_outputs(h, 2) == ERR_INVALID_ARGUMENT and L.sthip_outputs_ready(h, 2) == ERR_INVALID_ARGUMENT
        _assert_same(r.wait(t1), want, "first ticket")
        assert L.sthip_wait_outputs(h, t1) == 0 and r.ready(t1) and r.wait(t1) is None  # a double wait is fine
        # rejected, never ignored; the context still renders afterwards
        bufs = r.alloc_host_outputs(frame)
        pc = r.push_constants(frame)
        fd = frame.desc()
        ticket = C.c_uint64(99)

        def submit(o):
            return L.sthip_render_async(h, C.byref(pc), r.mSamplingFlags, sc.scene_flags, C.byref(fd), 0, 1, C.byref(o), C.byref(ticket))

        def outputs():
            o = wire.Outputs()
            o.gRadiance = wire.ptr(bufs["radiance"])
            return o

        o = outputs()
        o.device_ptrs = 1
        assert submit(o) == ERR_INVALID_ARGUMENT and ticket.value == 0 and b"device_ptrs" in L.sthip_last_error(h)
        o = outputs()
        o.debug_mode = 1
        dbg = np.zeros((64, 96, 4), np.float32)
        o.gDebugImage = wire.ptr(dbg)
        assert submit(o) == ERR_UNSUPPORTED and b"use sthip_render" in L.sthip_last_error(h)
        r.set_option("time_kernels", 1)
        assert submit(outputs()) == ERR_UNSUPPORTED and b"use sthip_render" in L.sthip_last_error(h)
        r.set_option("time_kernels", 0)
        _assert_same(r.wait(r.render_async(frame, 0, 1, host_outputs=bufs)), want, "after the rejections")
        # a scene upload, a ring change and a stream change with frames in flight complete them; the tickets stay waitable
        refs = [_copy(r.render(f, 10 + k, 1)) for k, f in enumerate(frames)]
        stream = torch.cuda.Stream()
        for drain in ("upload", "ring", "stream"):
            sets = [r.alloc_host_outputs(f) for f in frames[:2]]
            ts = [r.render_async(f, 10 + k, 1, host_outputs=sets[k]) for k, f in enumerate(frames[:2])]
            if drain == "upload":
                r.update(sc)
            elif drain == "ring":
                r.set_option("output_ring", 3)
            else:
                r.set_stream(stream.cuda_stream)
            for k in range(2):
                _assert_same(sets[k], refs[k], "%s: frame %d before its wait" % (drain, k))
            assert all(r.ready(t) for t in ts)
            for k, t in enumerate(ts):
                _assert_same(r.wait(t), refs[k], "%s: frame %d" % (drain, k))
        r.set_stream(0)
        r.set_option("output_ring", 2)
        # half_color_precision takes effect at the next submit; frames in flight keep the type they were submitted with
        pinned = [r.alloc_host_outputs(f) for f in frames]
        ts = [r.render_async(f, 10 + k, 1, host_outputs=pinned[k]) for k, f in enumerate(frames)]
        r.set_half_color_precision(True)
        half_t = r.render_async(frames[0], 10, 1)
        r.set_half_color_precision(False)
        for k, t in enumerate(ts):
            _assert_same(r.wait(t), refs[k], "in flight across the precision switch, frame %d" % k)
        got16 = r.wait(half_t)
        assert got16["radiance"].dtype == np.float16
        with np.errstate(over="ignore"):
            assert np.array_equal(got16["radiance"].view(np.uint16), refs[0]["radiance"].astype(np.float16).view(np.uint16))
        # destroy with frames in flight: the caller's buffers are complete afterwards (ordinary memory, which outlives close())
        sets = [_pageable_like(refs[k]) for k in range(3)]
        for k, f in enumerate(frames):
            r.render_async(f, 10 + k, 1, host_outputs=sets[k])
    finally:
        r.close()
    for k in range(3):
        _assert_same(sets[k], refs[k], "after destroy, frame %d" % k)


@pytest.mark.gpu
def test_destroy_completes_pinned_frames_in_flight(built, cornell):
    """sthip_destroy with two frames in flight into pinned memory of the caller's own (registered with the runtime through
    torch): no error, and the buffers hold the frames afterwards."""
    import ctypes as C

    import torch

    from stratum_amd import wire

    sc, cam = cornell
    frames = _moving_frames(cam, 2)
    r = _renderer(sc, ring=2)
    L = r._lib
    try:
        refs = [_copy(r.render(f, k, 1, aovs=False)) for k, f in enumerate(frames)]
        host = [torch.full((64, 96, 4), -1.0, dtype=torch.float32).pin_memory() for _ in frames]
        rays = [torch.zeros(2, dtype=torch.int64).pin_memory() for _ in frames]
        for k, f in enumerate(frames):
            pc, fd, o, t = r.push_constants(f), f.desc(), wire.Outputs(), C.c_uint64(0)
            o.gRadiance = host[k].data_ptr()
            o.gRayCount = rays[k].data_ptr()
            assert L.sthip_render_async(r._h, C.byref(pc), r.mSamplingFlags, sc.scene_flags, C.byref(fd), k, 1, C.byref(o), C.byref(t)) == 0
    finally:
        r.close()
    for k in range(2):
        assert np.array_equal(host[k].numpy().view(np.uint32), refs[k]["radiance"].view(np.uint32)), k
        assert np.array_equal(rays[k].numpy().astype(np.uint64), refs[k]["ray_count"]), k


@pytest.mark.gpu
def test_completion_happens_at_the_wait(async_host, tmp_path, cornell):
    """tests/cpp/async_host.cpp `gate`: with the render stream held by a host function, sthip_render_async returns,
    sthip_outputs_ready is 0 and the pinned buffers keep their fill; once the gate opens, sthip_wait_outputs delivers the
    synchronous frame. (A watchdog opens the gate after 20 s: a submit that synchronises fails cleanly.)"""
    from stratum_amd.scene import dump_description

    sc, cam = cornell
    desc = str(tmp_path / "scene.bin")
    dump_description(desc, sc, camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"]))
    out = subprocess.run(["timeout", "-k", "10", "120", async_host, "gate", desc], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("GATE OK"), out.stdout + out.stderr


@pytest.mark.gpu
def test_cpp_host_submit_finish_equals_render(async_host, tmp_path, cornell):
    """BDPT::submit / BDPT::finish over three frames of a sliding camera with two frames in flight = three BDPT::render calls:
    radiance, the tone-mapped result, prev-uv and the ray counts of prev_result(), frame by frame."""
    from stratum_amd.scene import dump_description

    sc, cam = cornell
    W, H = 96, 64
    desc = str(tmp_path / "scene.bin")
    dump_description(desc, sc, camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"]))
    raw = {}
    for mode in ("sync", "async"):
        outp = str(tmp_path / (mode + ".bin"))
        out = subprocess.run(["timeout", "-k", "10", "300", async_host, "frames", desc, outp, "2", mode], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.startswith("FRAMES OK " + mode), out.stdout + out.stderr
        raw[mode] = np.fromfile(outp, dtype=np.uint8)
    per_frame = W * H * (16 + 16 + 8) + 16
    assert raw["sync"].size == 3 * per_frame and raw["async"].size == raw["sync"].size
    s, a = raw["sync"].reshape(3, per_frame), raw["async"].reshape(3, per_frame)
    assert not np.array_equal(s[0], s[1]) and not np.array_equal(s[1], s[2])  # (the frames differ: a swapped order would show)
    for k in range(3):
        assert np.array_equal(s[k], a[k]), "frame %d" % k


@pytest.mark.gpu
def test_async_outputs_with_poisoned_allocations():
    """The identity and pipeline tests once more in a child process with STHIP_POISON_ALLOC (read once per process): every new
    device buffer — the staging sets of the ring among them — starts as 0x7F bytes, so a set that is copied before it is
    written shows."""
    if os.environ.get("STHIP_ASYNC_POISON_CHILD"):
        return  # (this is the child)
    env = dict(os.environ, STHIP_POISON_ALLOC="0x7F", STHIP_ASYNC_POISON_CHILD="1")
    out = subprocess.run(
        [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "equals_sync or pipeline"],
        env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500,
    )
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "failed" not in out.stdout
