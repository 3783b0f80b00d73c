"""The C++ host side (stratum_amd/host/stratum_hip.hpp): Stratum's Node graph / Scene / BDPT surface above the
C ABI. tests/cpp/host_test.cpp plays main.cpp: it builds the node graph from a scene description, lets
Application fire OnUpdate / OnRenderWindow, and is checked against the Python packing and renderer."""
import os
import subprocess

import numpy as np
import pytest

from stratum_amd import camera, scenes, wire
from stratum_amd.scene import SceneBuilder, dump_description, rotate_y, scale, translate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "host_test")


@pytest.fixture(scope="module")
def host_test(built):
    src = os.path.join(ROOT, "tests", "cpp", "host_test.cpp")
    hdr = os.path.join(ROOT, "stratum_amd", "host", "stratum_hip.hpp")
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(
            ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-o", EXE, src, "-L" + os.path.join(ROOT, "stratum_amd"), "-lstratum_hip", "-Wl,-rpath," + os.path.join(ROOT, "stratum_amd")]
        )
    return EXE


def foggy_cornell():
    import os

    return scenes.cornell_box(fog=np.load(os.path.join(os.path.dirname(__file__), "golden", "fog_sphere.npz"))["grid"], anisotropy=0.3)


def shared_mesh_scene():
    b = SceneBuilder("shared")
    m0 = b.add_material((0.7, 0.7, 0.7), roughness=0.3)
    m1 = b.add_material((0.2, 0.5, 0.9), metallic=0.8, roughness=0.2)
    li = b.add_emitter((9.0, 8.0, 7.0))
    q = scenes._quad((-1, 0, 1), (1, 0, 1), (1, 0, -1), (-1, 0, -1), (0, 1, 0))
    quad = b.add_mesh(*q, index_stride=2)
    for k in range(5):
        b.add_instance(quad, m0 if k % 2 else m1, translate((0.3 * k, 0.1 * k, -0.2 * k)) @ rotate_y(0.4 * k) @ scale((1.0 + 0.1 * k, 1.0, 0.7)))
    b.add_instance(quad, li, translate((0, 2.5, 0)) @ scale((0.5, 1.0, 0.5)) @ np.diag([1.0, -1.0, 1.0, 1.0]))
    return b.build(), {"eye": (0.5, 1.5, 4.0), "target": (0.5, 0.3, 0.0), "fovy": np.radians(50.0)}


@pytest.mark.parametrize("make", [scenes.cornell_box, shared_mesh_scene, scenes.textured_box, scenes.spheres_room, scenes.environment_scene, scenes.foliage, foggy_cornell])
def test_scene_update_packs_like_the_reference_layouts(host_test, tmp_path, make):
    sc, cam = make()
    fr = camera.Frame(64, 48, cam["fovy"], cam["eye"], cam["target"])
    desc = str(tmp_path / "scene.bin")
    dump_description(desc, sc, fr)
    out = subprocess.run([host_test, "pack", desc], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("PACK OK"), out.stdout + out.stderr


def bidirectional_cornell():
    return scenes.cornell_box()


BDPT_ARGS = {foggy_cornell: {"maxDiffuseVertices": 3}, bidirectional_cornell: {"bdptFlag": ["connectToLightPaths", "connecttoviews", "~deferShadowRays"], "maxDiffuseVertices": 3, "maxPathVertices": 6}}


@pytest.mark.gpu
@pytest.mark.parametrize("make", [scenes.cornell_box, shared_mesh_scene, scenes.textured_box, scenes.spheres_room, scenes.environment_scene, scenes.foliage, bidirectional_cornell, foggy_cornell])
def test_cpp_host_renders_what_the_python_host_renders(host_test, tmp_path, make):
    from stratum_amd.bdpt import BDPT
    from stratum_amd.post import Tonemapper, write_hdr

    sc, cam = make()
    args = BDPT_ARGS.get(make, {})
    argv = ["--%s=%s" % (k, x) for k, v in args.items() for x in (v if isinstance(v, list) else [v])]
    W, H, seeds = 96, 64, 3
    fr = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
    desc, outp = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    dump_description(desc, sc, fr)
    hdr = str(tmp_path / "image.hdr")
    out = subprocess.run([host_test, "render", desc, outp, str(seeds), str(wire.TONEMAP["ACES"]), "0.75", hdr] + argv, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("RENDER OK"), out.stdout + out.stderr
    raw = np.fromfile(outp, dtype=np.uint8)
    rad = raw[: W * H * 16].view(np.float32).reshape(H, W, 4)
    vis = raw[W * H * 16 : W * H * 24].view(wire.VisibilityInfo).reshape(H, W)
    rays = raw[W * H * 24 : W * H * 24 + 16].view(np.uint64)
    tm = raw[W * H * 24 + 16 :].view(np.float32).reshape(H, W, 4)
    r = BDPT(device=0, args=args)
    try:
        r.update(sc)
        ref = r.render(fr, 0, seeds)
        ref_tm = Tonemapper(r, "ACES", 0.75, True)(ref["radiance"])
    finally:
        r.close()
    assert np.array_equal(tm.view(np.uint32), ref_tm.view(np.uint32))
    write_hdr(tmp_path / "py.hdr", ref["radiance"])
    assert open(hdr, "rb").read() == (tmp_path / "py.hdr").read_bytes()
    assert np.array_equal(rad.view(np.uint32), ref["radiance"].view(np.uint32))
    assert np.array_equal(vis["instance_primitive_index"], ref["visibility"]["instance_primitive_index"])
    assert np.array_equal(rays, ref["ray_count"])


@pytest.mark.gpu
@pytest.mark.parametrize("flags, extra", [(["neereservoirs", "neereservoirreuse"], {"reservoirM": 2}),
                                          (["connecttolightpaths", "lightvertexcache", "lvcreservoirs", "lvcreservoirreuse"], {"lightPathCount": 3000, "reservoirM": 2, "maxDiffuseVertices": 3})])
def test_cpp_host_reuses_the_previous_frames_reservoirs(host_test, tmp_path, flags, extra):
    """A host that renders one frame per call: frame n looks into the hash grids frame n - 1 left (BDPT.cpp:482-483,621-627;
    `reuse_grids_persist`). The C++ host's third frame of an unchanged scene and camera is the third seed of the chain — the
    Python host's three one-seed calls with the option set, itself pinned to one call of three seeds in test_gpu_parity — and not
    the third seed rendered on its own."""
    from stratum_amd.bdpt import BDPT

    sc, cam = scenes.cornell_box()
    W, H = 96, 64
    fr = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
    desc, outp = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    dump_description(desc, sc, fr)
    argv = ["--bdptFlag=%s" % f for f in flags] + ["--%s=%s" % kv for kv in extra.items()] + ["--frames=3"]
    out = subprocess.run([host_test, "render", desc, outp, "1", "0", "0", str(tmp_path / "image.hdr")] + argv, capture_output=True, text=True)
    assert out.returncode == 0 and "FRAMES 3" in out.stdout, out.stdout + out.stderr
    raw = np.fromfile(outp + ".last", dtype=np.uint8)
    rad = raw[: W * H * 16].view(np.float32).reshape(H, W, 4)
    rays = raw[W * H * 16 :].view(np.uint64)
    r = BDPT(device=0, args=dict(extra, bdptFlag=flags))
    try:
        r.update(sc)
        alone = r.render(fr, 2, 1, aovs=False)
        r.set_option("reuse_grids_persist", 1)
        for seed in range(3):
            ref = r.render(fr, seed, 1, aovs=False)
    finally:
        r.close()
    assert np.array_equal(rad.view(np.uint32), ref["radiance"].view(np.uint32)) and np.array_equal(rays, ref["ray_count"])
    assert not np.array_equal(rad, alone["radiance"])


@pytest.mark.gpu
def test_cpp_host_moves_instances_with_a_top_level_rebuild(host_test, tmp_path):
    """Nodes move between two frames: Scene::update repacks (motion transforms from the previous frame's), BDPT::update
    finds only transforms changed and calls sthip_scene_update_transforms; the second frame and its prev-uv output equal
    what the Python host gets from SceneData.set_instance_transform + BDPT.update_transforms."""
    from stratum_amd.bdpt import BDPT
    from stratum_amd.scene import translate

    sc, cam = scenes.cornell_box()
    W, H, seeds = 96, 64, 2
    fr = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
    desc, outp = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    dump_description(desc, sc, fr)
    out = subprocess.run([host_test, "render", desc, outp, str(seeds), "0", "0", str(tmp_path / "x.hdr"), "--move=0.1,0.0,-0.15"], capture_output=True, text=True)
    assert out.returncode == 0 and "MOVED transforms_only=1" in out.stdout, out.stdout + out.stderr
    raw = np.fromfile(outp + ".moved", dtype=np.float32)
    rad, prev_uv = raw[: W * H * 4].reshape(H, W, 4), raw[W * H * 4 :].reshape(H, W, 2)
    r = BDPT(device=0)
    try:
        r.update(sc)
        r.render(fr, 0, seeds)
        moved = [i for i in range(sc.instances.shape[0]) if not np.array_equal(sc.transforms["m"][i], np.eye(4, dtype=np.float32)[:3])]
        assert len(moved) == 2  # the two blocks
        for i in moved:
            m = sc.transforms["m"][i].copy()
            m[:, 3] += np.array([0.1, 0.0, -0.15], np.float32)  # float32 adds, as the C++ node transform is moved
            sc.set_instance_transform(i, m)
        r.update_transforms(sc)
        ref = r.render(fr, seeds, seeds)  # the C++ host's frame number went on: seeds `seeds` .. 2 seeds - 1
    finally:
        r.close()
    assert np.array_equal(rad.view(np.uint32), ref["radiance"].view(np.uint32))
    assert np.array_equal(prev_uv.view(np.uint32), ref["prev_uv"].view(np.uint32))


# ---- the plugin boundary: `--plugin=libstratum_hip_plugin.so;stratum_hip_register` (main.cpp:11-24,148-149) ----
def _plugin_host(built, spec):
    import __graft_entry__ as g

    g.build_plugin()
    return subprocess.run([g.PLUGIN_HOST, spec], capture_output=True, text=True)


def test_plugin_loads_and_its_entry_point_runs(built):
    """dlopen(RTLD_NOW) of the plugin resolves every symbol (it links libstratum_hip.so by $ORIGIN), dlsym finds the entry
    point, and calling it with a stm::Node& constructs the renderer — which needs a HIP device: on a box without one the
    only acceptable outcome is the sthip_create error (exit 3), never a load failure or a missing symbol."""
    import __graft_entry__ as g

    out = _plugin_host(built, g.PLUGIN + ";stratum_hip_register")
    assert out.returncode in (0, 3), out.stdout + out.stderr
    assert ("PLUGIN OK" in out.stdout) if out.returncode == 0 else ("sthip_create" in out.stdout)


def test_plugin_loader_errors_are_the_references(built):
    """dynamic_library.hpp:29,50: a library that does not load throws runtime_error, a missing symbol invalid_argument."""
    import __graft_entry__ as g

    out = _plugin_host(built, g.PLUGIN + ";no_such_entry_point")
    assert out.returncode == 4 and "Could not find function no_such_entry_point" in out.stdout
    out = _plugin_host(built, "/nonexistent/libnope.so;stratum_hip_register")
    assert out.returncode == 5 and "Failed to load /nonexistent/libnope.so" in out.stdout


@pytest.mark.gpu
def test_plugin_installs_the_renderer_on_a_gpu(built):
    import __graft_entry__ as g

    out = _plugin_host(built, g.PLUGIN + ";stratum_hip_register")
    assert out.returncode == 0 and "PLUGIN OK" in out.stdout, out.stdout + out.stderr


def test_packed_node_planes_are_conservative(tmp_path):
    """The 48-byte node (bvh.h: BvhNodePacked) keeps its child references in the low mantissa byte of eight planes;
    tests/cpp/pack_test.cpp checks that pack_plane's outward rounding keeps every plane conservative for EVERY byte value,
    finite, within 511 ulp, and that references round-trip (200 k random + special values, host only)."""
    exe = str(tmp_path / "pack_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tests", "cpp", "pack_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("PACK OK"), out.stdout + out.stderr


def test_shade_variant_rule_matches_the_instantiation_lists(tmp_path):
    """csrc/kernel_variants.h: the rule that picks k_shade's template arguments selects only listed instantiations, every
    listed one is selected by some reachable input, and rule and LDS size agree with the former if/else ladders written out
    in tests/cpp/kernel_variants_check.cpp (host only: the header has no HIP in it)."""
    exe = str(tmp_path / "kernel_variants_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "kernel_variants_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("VARIANTS OK: 24 listed, 24 selected"), out.stdout + out.stderr


# ---- the multi-GPU driver of the C++ host (host/stratum_hip_multi.hpp) ----
def _multi_host(built):
    import __graft_entry__ as g

    return g.build_multi_host()


@pytest.mark.parametrize("w,h,world,tw,th", [(1920, 1080, 8, 64, 32), (100, 70, 3, 16, 8), (64, 32, 4, 64, 32), (3840, 2160, 8, 64, 32)])
def test_cpp_shard_layout_is_the_python_and_device_layout(built, w, h, world, tw, th):
    """stm::ShardLayout (owner rule, slot -> pixel, host assembly) against stratum_amd.shard, the mirror the device
    kernels are tested against: same slot counts, same pixel per slot; packing by ownership and assembling is lossless.
    This is the N-rank logic of MultiDeviceBDPT without N GPUs."""
    from stratum_amd import shard

    out = subprocess.run([_multi_host(built), "layout", str(w), str(h), str(world), str(tw), str(th)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("LAYOUT OK"), out.stdout + out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("rank")]
    assert len(lines) == world
    for rank, ln in enumerate(lines):
        assert int(ln[3]) == shard.slot_count(w, h, rank, world, tw, th)
        xy = shard.slot_pixels(w, h, rank, world, tw, th)
        s = 0
        for x, y in xy:  # the same FNV-style fold the program prints
            s = (s * 1099511628211 + (int(y) * w + int(x) + 1 if x >= 0 else 0)) & 0xFFFFFFFFFFFFFFFF
        assert int(ln[5]) == s


@pytest.fixture(scope="module")
def multi_mock_exe(tmp_path_factory):
    """tests/cpp/multi_mock.cpp: the C++ multi-GPU driver over stand-ins for the C ABI, HIP and RCCL (no GPU, no libraries)."""
    exe = str(tmp_path_factory.mktemp("multi_mock") / "multi_mock")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "multi_mock.cpp"), "-lpthread"])
    return exe


@pytest.mark.parametrize("world,w,h,tw,th", [(2, 192, 96, 64, 32), (3, 100, 70, 16, 8), (5, 200, 120, 64, 32), (8, 320, 200, 64, 32), (8, 64, 32, 64, 32)])
def test_cpp_multi_device_driver_at_world_2_to_8_over_stand_ins(multi_mock_exe, tmp_path, world, w, h, tw, th):
    """stm::MultiDeviceBDPT with N ranks and no GPU: its persistent rank threads, both phases of a frame, the packing of the
    G-buffer outputs, the send / recv exchange, the assembly through ShardLayout, frames in flight and seed bookkeeping run
    over host stand-ins for sthip_*, hip* and nccl* (tests/cpp/multi_mock.cpp). A rank that fails makes render() throw
    BEFORE any collective is posted (the old single-phase form left the other ranks waiting for ever), and the
    driver renders the next frame as if nothing had happened. Frames larger and smaller than a tile round, ragged edges."""
    sc, cam = scenes.cornell_box()
    fr = camera.Frame(w, h, cam["fovy"], cam["eye"], cam["target"])
    desc = str(tmp_path / "scene.bin")
    dump_description(desc, sc, fr)
    out = subprocess.run([multi_mock_exe, desc, str(world), str(tw), str(th)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and ("MULTI MOCK OK world %d" % world) in out.stdout, out.stdout + out.stderr[-2000:]


def test_cpp_multi_device_driver_under_thread_sanitizer(tmp_path):
    """The same program under ThreadSanitizer at world 4: the rank threads' job hand-over, the frames in flight and the
    failure path hold no data race."""
    exe = str(tmp_path / "multi_mock_tsan")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "multi_mock.cpp"), "-lpthread"])
    sc, cam = scenes.cornell_box()
    desc = str(tmp_path / "scene.bin")
    dump_description(desc, sc, camera.Frame(160, 100, cam["fovy"], cam["eye"], cam["target"]))
    out = subprocess.run([exe, desc, "4", "32", "16"], capture_output=True, text=True, timeout=600, env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1"))
    assert out.returncode == 0 and "MULTI MOCK OK world 4" in out.stdout and "ThreadSanitizer" not in out.stderr, out.stdout + out.stderr[-3000:]


@pytest.mark.gpu
def test_cpp_multi_device_driver_seed_split_on_one_gpu(built, tmp_path):
    """MultiDeviceBDPT::split_seeds with the one GPU of this box: the whole frame rendered for the call's seeds, turned into
    sums (sthip_radiance_to_sums), reduced with the real ncclReduce(sum) and turned back: the single-device frame up to the
    rounding of (mean * n) / n; light tracing's splats — refused on a tile shard of more than one rank — go through it."""
    from stratum_amd.bdpt import BDPT

    sc, cam = scenes.cornell_box()
    W, H, seeds = 192, 96, 3
    fr = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
    desc, outp = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    dump_description(desc, sc, fr)
    for extra, args in (([], {}), (["--bdptFlag=connecttoviews"], {"bdptFlag": ["connecttoviews"]})):
        out = subprocess.run([_multi_host(built), "render", desc, outp, str(seeds), "0", "--splitSeeds=1"] + extra, capture_output=True, text=True)
        assert out.returncode == 0 and "RENDER OK world 1" in out.stdout, out.stdout + out.stderr
        raw = np.fromfile(outp, dtype=np.uint8)
        rad = raw[: W * H * 16].view(np.float32).reshape(H, W, 4)
        rays = raw[W * H * 16 : W * H * 16 + 16].view(np.uint64)
        r = BDPT(device=0, args=args)
        try:
            r.update(sc)
            ref = r.render(fr, 0, seeds)
        finally:
            r.close()
        assert np.array_equal(rad[..., 3], ref["radiance"][..., 3])
        np.testing.assert_allclose(rad[..., :3], ref["radiance"][..., :3], rtol=3e-7, atol=0)
        assert np.array_equal(rays, ref["ray_count"])


@pytest.mark.gpu
@pytest.mark.parametrize("make", [scenes.cornell_box, shared_mesh_scene])
def test_cpp_multi_device_driver_on_one_gpu(built, tmp_path, make):
    """MultiDeviceBDPT with the one GPU of this box: its whole path runs (one thread per rank, packed tiles, the RCCL
    send / recv group, sthip_assemble_tiles on rank 0) and the frame equals the single-device renderer's bit for bit."""
    from stratum_amd.bdpt import BDPT

    sc, cam = make()
    W, H, seeds = 192, 96, 3
    fr = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
    desc, outp = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    dump_description(desc, sc, fr)
    out = subprocess.run([_multi_host(built), "render", desc, outp, str(seeds), "0"], capture_output=True, text=True)
    assert out.returncode == 0 and "RENDER OK world 1" in out.stdout, out.stdout + out.stderr
    raw = np.fromfile(outp, dtype=np.uint8)
    rad = raw[: W * H * 16].view(np.float32).reshape(H, W, 4)
    rays = raw[W * H * 16 : W * H * 16 + 16].view(np.uint64)
    r = BDPT(device=0)
    try:
        r.update(sc)
        ref = r.render(fr, 0, seeds)
    finally:
        r.close()
    assert np.array_equal(rad.view(np.uint32), ref["radiance"].view(np.uint32))
    assert np.array_equal(rays, ref["ray_count"])


@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_host_bvh_builder_under_sanitizers(tmp_path, sanitizer):
    """stratum_amd/csrc/bvh_build.cpp on the CPU under ASan + UBSan and under TSan (the bottom levels are built by a pool of
    threads; GPU sanitizers are not available on the pool): validation, binned SAH, embedded leaves, top level,
    transforms-only rebuild, treetop, node packing — on a merged mesh (atrium), shared instanced meshes (forest) and
    spheres / tiny meshes; tests/cpp/bvh_host_check.cpp checks that every reference stays in range and every triangle
    is referenced."""
    from stratum_amd import scenes

    exe = str(tmp_path / "bvh_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=" + sanitizer, "-o", exe, os.path.join(ROOT, "tests", "cpp", "bvh_host_check.cpp"),
                           os.path.join(ROOT, "stratum_amd", "csrc", "bvh_build.cpp"), "-lpthread"])
    for name, (sc, _) in (("atrium", scenes.atrium(target_tris=60000)), ("forest", scenes.forest(n_instances=40, tree_tris=900, tree_kinds=3)), ("spheres", scenes.spheres_room())):
        d = tmp_path / name
        d.mkdir()
        for arr, fn in ((sc.vertices, "vertices"), (sc.indices, "indices"), (sc.instances, "instances"), (sc.transforms, "xf"), (sc.inverse_transforms, "inv_xf"), (sc.materials, "materials")):
            np.ascontiguousarray(arr).tofile(str(d / (fn + ".bin")))
        env = dict(os.environ, STHIP_BUILD_THREADS="6", ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1", TSAN_OPTIONS="halt_on_error=1")
        out = subprocess.run([exe, str(d)], capture_output=True, text=True, env=env)
        assert out.returncode == 0 and "BVH HOST OK" in out.stdout, name + ": " + out.stdout + out.stderr[-3000:]


# ---------------------------------------------------------------------------------------------------------------------------
# The host part of the upload (stratum_amd/csrc/scene_prepare.cpp) under ASan + UBSan: tests/cpp/scene_prepare_check.cpp
# ---------------------------------------------------------------------------------------------------------------------------
F32 = np.float32
DEVICE_IMAGE = np.dtype([("offset", "<u4", (16,)), ("w", "<u2", (16,)), ("h", "<u2", (16,)), ("levels", "<u4"), ("format", "<u4"), ("pad", "<u4", (2,))])
DEVICE_IMAGE1 = np.dtype([("offset", "<u4"), ("w", "<u4"), ("h", "<u4"), ("format", "<u4")])
EMITTER_BOUNDS = np.dtype([("lo", "<f4", (3,)), ("instance", "<u4"), ("hi", "<f4", (3,)), ("identity", "<u4"), ("sphere", "<f4", (4,))])
INVALID = -1  # STHIP_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def scene_prepare_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("scene_prepare") / "scene_prepare_check")
    csrc = os.path.join(ROOT, "stratum_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "scene_prepare_check.cpp"), os.path.join(csrc, "scene_prepare.cpp"), os.path.join(csrc, "bvh_build.cpp"), "-lpthread"])
    return exe


def _image_entries(images):
    """(width, height, format, payload) per image as scene_prepare_check reads them: uint8 arrays are the 8-bit formats"""
    return [(im.shape[1], im.shape[0], 1 if im.dtype == np.uint8 else 0, im) for im in images]


def _dump_arrays(d, sc, images=None, masks=None, volumes=None):
    """The scene arrays of `sc` into directory `d`; images / masks / volumes override what the scene holds with explicit
    entries (so that a descriptor can state what no array could hold: a width of 65536, 16 GiB of grids)"""
    d.mkdir()
    for arr, fn in ((sc.vertices, "vertices"), (sc.indices, "indices"), (sc.instances, "instances"), (sc.transforms, "xf"), (sc.inverse_transforms, "inv_xf"), (sc.materials, "materials"),
                    (sc.lights.astype(np.uint32), "lights"), (sc.distributions.astype(F32), "distributions")):
        np.ascontiguousarray(arr).tofile(str(d / (fn + ".bin")))
    for fn, entries in (("images", _image_entries(sc.images) if images is None else images), ("masks", _image_entries(sc.images1) if masks is None else masks)):
        with open(str(d / (fn + ".bin")), "wb") as f:
            f.write(np.uint32(len(entries)).tobytes())
            for w, h, fmt, payload in entries:
                data = b"" if payload is None else np.ascontiguousarray(payload).tobytes()
                f.write(np.array([w, h, fmt], np.uint32).tobytes() + np.uint64(len(data)).tobytes() + data)
    with open(str(d / "volumes.bin"), "wb") as f:
        entries = [(g.nbytes, g) for g in sc.volumes] if volumes is None else volumes
        f.write(np.uint32(len(entries)).tobytes())
        for stated, payload in entries:
            data = np.ascontiguousarray(payload).tobytes()
            f.write(np.array([stated, len(data)], np.uint64).tobytes() + data)
    return str(d)


def _run_prepare(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe] + list(args), capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    return out.stdout


def _sphere_and_quad():
    b = SceneBuilder("sphere_and_quad")
    quad = b.add_mesh(*scenes._quad((-1, 0, 1), (1, 0, 1), (1, 0, -1), (-1, 0, -1), (0, 1, 0)))
    b.add_instance(quad, b.add_material((0.7, 0.7, 0.7), roughness=0.3))
    b.add_sphere(b.add_material((0.2, 0.5, 0.9), roughness=0.4), 0.5, translate((0, 1, 0)))
    return b.build()


def _record(sc, instance):
    """the material record of an instance, as a writable view into the scene's material bytes"""
    address = int(sc.instances["packed"][instance, 0]) >> 4
    return sc.materials[address : address + wire.MaterialRecord.itemsize].view(wire.MaterialRecord)[0]


def _rejections():
    """(name, make scene, defect(sc) -> dump overrides or None, arguments, message): a valid scene with exactly one defect. The
    messages are those of the upload before its checks moved into check_scene, copied here."""
    cornell = lambda: scenes.cornell_box()[0]
    textured = lambda: scenes.textured_box()[0]
    foliage = lambda: scenes.foliage()[0]
    foggy = lambda: foggy_cornell()[0]
    env = lambda: scenes.environment_scene()[0]
    cases = []
    add = lambda name, make, defect, args, message: cases.append((name, make, defect, args, message))
    required = "scene: a required array is NULL or there are no instances"
    for a in ("scene", "gInstances", "gInstanceTransforms", "gInstanceInverseTransforms", "gMaterialData"):
        add("null_" + a, cornell, None, ["null:" + a], required)

    def no_instances(sc):
        sc.instances = sc.instances[:0]

    add("no_instances", cornell, no_instances, [], required)
    for a in ("gVertices", "gIndices"):
        add("null_" + a, cornell, None, ["null:" + a], "scene: vertex_count / indices_bytes > 0 but the array is NULL")

    def many_instances(sc):
        reps = 65536 // sc.instances.shape[0] + 1
        sc.instances, sc.transforms, sc.inverse_transforms = (np.tile(a, reps)[:65536] for a in (sc.instances, sc.transforms, sc.inverse_transforms))

    add("65536_instances", cornell, many_instances, [], "scene: more than 65535 instances (16-bit instance index, scene.h:23)")
    add("null_gLightInstances", cornell, None, ["null:gLightInstances"], "scene: light_count > 0 but gLightInstances is NULL")

    def image_format_2(sc):
        e = _image_entries(sc.images)
        e[0] = e[0][:2] + (2,) + e[0][3:]
        return {"images": e}

    def mask_format_2(sc):
        e = _image_entries(sc.images1)
        e[0] = e[0][:2] + (2,) + e[0][3:]
        return {"masks": e}

    add("image_format_2", textured, image_format_2, [], "scene: image_formats[0] = 2 is not a format of gImages")
    add("mask_format_2", foliage, mask_format_2, [], "scene: image1_formats[0] = 2 is not a format of gImage1s")

    def light_out_of_range(sc):
        sc.lights[0] = sc.instances.shape[0]

    add("light_out_of_range", cornell, light_out_of_range, [], "scene: gLightInstances entry out of range")
    add("null_gImages", textured, None, ["null:gImages"], "scene: image_count > 0 but gImages is NULL")

    def medium_of(sc):
        return int(np.nonzero((sc.instances["packed"][:, 0] & 0xF) == wire.INSTANCE_TYPE_VOLUME)[0][0])

    def medium_address(sc):
        sc.instances["packed"][medium_of(sc), 0] = ((sc.materials.size - 36) << 4) | wire.INSTANCE_TYPE_VOLUME

    def medium_misaligned(sc):
        sc.instances["packed"][medium_of(sc), 0] += 2 << 4
        sc.materials = np.concatenate([sc.materials, np.zeros(4, np.uint8)])

    def medium_volume(sc):
        address = int(sc.instances["packed"][medium_of(sc), 0]) >> 4
        sc.materials[address + 32 : address + 36] = np.array([len(sc.volumes)], np.uint32).view(np.uint8)

    add("medium_address", foggy, medium_address, [], "scene: medium material_address out of range")
    add("medium_misaligned", foggy, medium_misaligned, [], "scene: medium material_address out of range")
    add("medium_volume", foggy, medium_volume, [], "scene: a medium refers to a volume that is not in gVolumes")

    def material_address(sc):
        sc.instances["packed"][0, 0] = (sc.materials.size - wire.MaterialRecord.itemsize + 4) << 4

    add("material_address", cornell, material_address, [], "scene: material_address out of range")
    for k in range(3):
        def image_index(sc, k=k):
            _record(sc, 0)["values"]["image_index"][k] = len(sc.images)

        add("image_index_%d" % k, textured, image_index, [], "scene: a material refers to an image that is not in gImages")

    def bump_index(sc):
        _record(sc, 0)["bump_index"] = len(sc.images)

    add("bump_index", textured, bump_index, [], "scene: a bump map refers to an image that is not in gImages")

    def alpha_index(instance):
        def defect(sc):
            _record(sc, instance)["alpha_mask_index"] = len(sc.images1)

        return defect

    add("alpha_index_foliage", foliage, lambda sc: alpha_index(int(np.nonzero([_record(sc, i)["alpha_mask_index"] < 4096 for i in range(sc.instances.shape[0])])[0][0]))(sc), [],
        "scene: a material refers to an alpha mask that is not in gImage1s")
    add("alpha_index_triangles", _sphere_and_quad, alpha_index(0), [], "scene: a material refers to an alpha mask that is not in gImage1s")
    add("alpha_index_sphere", _sphere_and_quad, alpha_index(1), [], None)  # (a sphere has no uv to test a mask at: accepted)
    add("null_gImage1s", foliage, None, ["null:gImage1s"], "scene: image1_count > 0 but gImage1s is NULL")
    add("null_gVolumes", foggy, None, ["null:gVolumes"], "scene: volume_count > 0 but gVolumes is NULL")
    add("null_gDistributions", env, None, ["null:gDistributions"], "scene: distribution_count > 0 but gDistributions is NULL")

    def bad_image(which, w=None, h=None, pixels=True):
        def defect(sc):
            e = _image_entries(sc.images if which == "images" else sc.images1)
            texel = np.zeros(4, F32)  # (the check looks at the descriptor only)
            e[0] = (e[0][0] if w is None else w, e[0][1] if h is None else h, 0, texel if pixels else None)
            return {which: e}

        return defect

    add("image_0_wide", textured, bad_image("images", w=0), [], "scene: bad image")
    add("image_0_high", textured, bad_image("images", h=0), [], "scene: bad image")
    add("image_65536_wide", textured, bad_image("images", w=65536), [], "scene: bad image")
    add("image_65536_high", textured, bad_image("images", h=65536), [], "scene: bad image")
    add("image_no_pixels", textured, bad_image("images", pixels=False), [], "scene: bad image")
    add("mask_0_wide", foliage, bad_image("masks", w=0), [], "scene: bad alpha-mask image")
    add("mask_65536_high", foliage, bad_image("masks", h=65536), [], "scene: bad alpha-mask image")
    add("mask_no_pixels", foliage, bad_image("masks", pixels=False), [], "scene: bad alpha-mask image")
    add("volumes_16_gib", foggy, lambda sc: {"volumes": [(1 << 34, g) for g in sc.volumes]}, [], "scene: gVolumes exceed 16 GiB")
    add("valid_cornell", cornell, None, [], None)
    add("valid_foggy", foggy, None, [], None)
    return cases


def test_check_scene_refuses_what_the_upload_refused(scene_prepare_check, tmp_path):
    """Every refusal that moved from scene_upload into check_scene: a small valid scene with exactly that defect gets the code
    and the message, byte for byte, that the upload gave it before the move."""
    for name, make, defect, args, message in _rejections():
        sc = make()
        overrides = (defect(sc) if defect else None) or {}
        out = _run_prepare(scene_prepare_check, "check", _dump_arrays(tmp_path / name, sc, **overrides), *args)
        assert out == ("ACCEPTED\n" if message is None else "REFUSED %d\n%s\n" % (INVALID, message)), name + ": " + out


# ---- the numpy restatement of scene_prepare.cpp's arithmetic: float32, the same operations in the same order ----
def _texel_range(image, channel):
    t = image[..., channel].reshape(-1)
    t = t.astype(F32) / F32(255) if image.dtype == np.uint8 else t
    if t.size == 0 or np.isnan(t).any():
        return F32(-np.inf), F32(np.inf)
    return t.min(), t.max()


def _value_range(sc, rec, k, channel):
    c = F32(rec["values"]["value"][k][channel])
    index = int(rec["values"]["image_index"][k])
    if index >= 4096 or index >= len(sc.images):
        return c, c
    if not np.any(rec["values"]["value"][k] > 0):
        return F32(0), F32(0)
    a, b = _texel_range(sc.images[index], channel)
    with np.errstate(invalid="ignore"):
        pa, pb = F32(c * a), F32(c * b)
    lo, hi = (pb if pb < pa else pa), (pb if pa < pb else pa)  # std::min / std::max
    if np.isnan(lo) or np.isnan(hi):
        return F32(-np.inf), F32(np.inf)
    return lo, hi


def _analyse(sc):
    n = sc.instances.shape[0]
    flags = np.full(max(1, n), 0x80, np.uint8)
    is_volume = np.zeros(n, np.uint8)
    specular = textured = alpha = spheres = False
    for i in range(n):
        kind, address = int(sc.instances["packed"][i, 0]) & 0xF, int(sc.instances["packed"][i, 0]) >> 4
        spheres |= kind == wire.INSTANCE_TYPE_SPHERE
        if kind == wire.INSTANCE_TYPE_VOLUME:
            is_volume[i] = 1
            specular |= not (abs(sc.materials[address + 12 : address + 16].view(F32)[0]) <= F32(0.999))
            continue
        rec = sc.materials[address : address + wire.MaterialRecord.itemsize].view(wire.MaterialRecord)[0]
        textured |= bool(np.any(rec["values"]["image_index"] < 4096)) or rec["bump_index"] < 4096
        alpha |= rec["alpha_mask_index"] < 4096 and kind == wire.INSTANCE_TYPE_TRIANGLES
        metallic_hi, roughness_lo, transmission_hi = _value_range(sc, rec, 1, 0)[1], _value_range(sc, rec, 1, 1)[0], _value_range(sc, rec, 2, 2)[1]
        specular |= bool((metallic_hi > F32(0.999) or transmission_hi > F32(0.999)) and roughness_lo <= F32(1e-2))
        f = sc.materials[address : address + 56].view(F32)
        le = [F32(f[k] * f[3]) for k in range(3)]
        emits, can_eval = any(v > 0 for v in le), f[3] <= 0 and any(f[k] > 0 for k in range(3))
        flags[i] = (1 if emits else 0) | (2 if can_eval else 0) | (4 if (f[5] > F32(0.999) or f[12] > F32(0.999)) and f[6] <= F32(1e-2) else 0)
    return np.array([specular, textured, alpha, spheres, bool(is_volume.any())], np.uint8), flags, is_volume


def _layout_images(images):
    table, texels, words8 = np.zeros(len(images), DEVICE_IMAGE), [], 0
    floats = 0  # float4 texels so far
    for i, im in enumerate(images):
        h, w = im.shape[:2]
        level = im
        for k in range(16):
            table[i]["offset"][k], table[i]["w"][k], table[i]["h"][k], table[i]["levels"] = (words8 if im.dtype == np.uint8 else floats), w, h, k + 1
            if im.dtype == np.uint8:
                table[i]["format"] = 1
                words8 += w * h
            else:
                texels.append(level.reshape(-1))
                floats += w * h
            if (w == 1 and h == 1) or k == 15:
                break
            nw, nh = max(1, w // 2), max(1, h // 2)
            if im.dtype != np.uint8:
                x0, x1 = np.minimum(2 * np.arange(nw), w - 1), np.minimum(2 * np.arange(nw) + 1, w - 1)
                y0, y1 = np.minimum(2 * np.arange(nh), h - 1), np.minimum(2 * np.arange(nh) + 1, h - 1)
                a, b, c, e = level[y0][:, x0], level[y0][:, x1], level[y1][:, x0], level[y1][:, x1]
                level = (((a + b) + (c + e)) * F32(0.25)).astype(F32)
            w, h = nw, nh
    return table, (np.concatenate(texels) if texels else np.zeros(0, F32)), np.uint64(words8)


def _layout_masks(masks):
    table, texels, texels8 = np.zeros(len(masks), DEVICE_IMAGE1), [np.zeros(0, F32)], [np.zeros(0, np.uint8)]
    for i, im in enumerate(masks):
        own = texels8 if im.dtype == np.uint8 else texels
        table[i] = (sum(t.size for t in own), im.shape[1], im.shape[0], 1 if im.dtype == np.uint8 else 0)
        own.append(im.reshape(-1))
    return table, np.concatenate(texels), np.concatenate(texels8)


def _emitters(sc, flags):
    out = []
    ident = np.eye(4, dtype=F32)[:3]
    for i in range(sc.instances.shape[0]):
        p = [int(v) for v in sc.instances["packed"][i]]
        if (p[0] & 0xF) != wire.INSTANCE_TYPE_TRIANGLES or not (flags[i] & 1):
            continue
        if len(out) == 16:
            return np.zeros(0, EMITTER_BOUNDS)
        prims, stride = (p[1] >> 12) & 0xFFFF, p[1] >> 28
        index = sc.indices[p[3] : p[3] + 3 * prims * stride].view("<u2" if stride == 2 else "<u4").astype(np.int64)
        pos = sc.vertices["position"][p[2] + index]
        b = np.zeros((), EMITTER_BOUNDS)
        lo, hi = pos.min(axis=0), pos.max(axis=0)
        mag = (np.maximum(np.abs(lo), np.abs(hi)) * (F32(1.0) / F32(32768.0)) + F32(1e-30)).astype(F32)
        lo, hi = (lo - mag).astype(F32), (hi + mag).astype(F32)
        b["lo"], b["hi"], b["instance"] = lo, hi, i
        b["sphere"][:3] = F32(0.5) * lo + F32(0.5) * hi
        b["sphere"][3] = F32(np.sqrt(np.sum((hi.astype(np.float64) - lo.astype(np.float64)) ** 2)))
        b["identity"] = np.array_equal(sc.transforms["m"][i], ident) and np.array_equal(sc.inverse_transforms["m"][i], ident)
        out.append(b)
    return np.array(out, EMITTER_BOUNDS) if out else np.zeros(0, EMITTER_BOUNDS)


def _expect(d, sc, what=("analysis", "images", "masks", "emitters", "volumes")):
    """writes the restatement's results for `sc` beside the dumped arrays; the program compares bytes"""
    flags5, inst_flags, is_volume = _analyse(sc)
    results = {}
    if "analysis" in what:
        results.update(scene_flags=flags5, inst_flags=inst_flags, instance_is_volume=is_volume, volume_instances=np.uint32(is_volume.sum()))
    if "images" in what:
        results["image_table"], results["image_texels"], results["image_words8"] = _layout_images(sc.images)
    if "masks" in what:
        results["mask_table"], results["mask_texels"], results["mask_texels8"] = _layout_masks(sc.images1)
    if "emitters" in what:
        results["emitters"] = _emitters(sc, inst_flags)
        results["emitter_count"] = np.uint32(results["emitters"].shape[0])
    if "volumes" in what:
        words = [g.nbytes // 4 for g in sc.volumes]
        results["volume_first_words"], results["volume_words"] = np.cumsum([0] + words)[:-1].astype(np.uint32), np.uint64(sum(words))
    for name, value in results.items():
        np.ascontiguousarray(value).tofile(os.path.join(d, "expect_%s.bin" % name))
    return results


def _one_quad(material):
    """a scene of one quad whose material `material(builder)` makes"""
    b = SceneBuilder("one_quad")
    b.add_instance(b.add_mesh(*scenes._quad((-1, 0, 1), (1, 0, 1), (1, 0, -1), (-1, 0, -1), (0, 1, 0))), material(b))
    return b.build()


def _params_material(texture, metallic=1.0, roughness=0.005):
    def make(b):
        m = b.add_material((0.8, 0.8, 0.8), metallic=metallic, roughness=roughness)
        b.set_material_images(m, params_image=b.add_image(texture))
        return m

    return make


def _prepared_scenes():
    """(name, scene, has_specular the case is there to show or None)"""
    out = [(make.__name__, make()[0], None) for make in (scenes.cornell_box, scenes.textured_box, scenes.spheres_room, scenes.environment_scene, scenes.foliage, foggy_cornell, shared_mesh_scene)]
    out.append(("textured_box_mirror_map", scenes.textured_box(mirror_map=True)[0], 1))
    # has_specular: what constant * texel can reach over the image's texels
    rough0, rough1 = np.ones((2, 3, 4), F32), np.ones((2, 3, 4), F32)
    rough0[1, 2, 1] = 0
    nan = rough1.copy()
    nan[0, 1, 1] = np.nan
    out.append(("metal_roughness_texel_0", _one_quad(_params_material(rough0)), 1))
    out.append(("metal_roughness_texel_1", _one_quad(_params_material(rough1)), 1))  # (0.005 * 1 is still <= 0.01)
    out.append(("metal_rough_texel_0", _one_quad(_params_material(rough0, roughness=0.5)), 1))
    out.append(("metal_rough_texel_1", _one_quad(_params_material(rough1, roughness=0.5)), 0))
    out.append(("metal_rough_nan_texel", _one_quad(_params_material(nan, roughness=0.5)), 1))
    out.append(("no_positive_component", _one_quad(_params_material(rough0, metallic=0.0, roughness=0.0)), 0))
    out.append(("metal_rough_byte_0", _one_quad(_params_material((rough0 * 255).astype(np.uint8), roughness=0.5)), 1))
    out.append(("metal_rough_byte_255", _one_quad(_params_material((rough1 * 255).astype(np.uint8), roughness=0.5)), 0))
    # the mip chains: odd sizes (the min(2x + 1, w - 1) clamp), 65535 x 1 (16 levels: the STHIP_MAX_MIPS stop and the 1 x 1 stop
    # coincide), float and RGBA8 images interleaved (two offset counters)
    rng = np.random.default_rng(7)
    sc = scenes.cornell_box()[0]
    sc.images = []
    for k, (w, h) in enumerate([(1, 1), (2, 2), (3, 5), (5, 3), (1, 7), (7, 1), (65535, 1)]):
        sc.images.append(rng.random((h, w, 4), dtype=F32) * F32(4))
        if k % 2 == 0:
            sc.images.append(rng.integers(0, 256, (min(w, 8) + 1, h + 2, 4), dtype=np.uint8))
    sc.images1 = [rng.random((2, 3), dtype=F32), rng.integers(0, 256, (3, 5), dtype=np.uint8), rng.random((1, 1), dtype=F32), rng.integers(0, 256, (2, 2), dtype=np.uint8)]
    out.append(("mip_chains_and_masks", sc, None))
    # 17 emitters: one more than the table holds, so there is no table
    b = SceneBuilder("emitters17")
    quad = b.add_mesh(*scenes._quad((-1, 0, 1), (1, 0, 1), (1, 0, -1), (-1, 0, -1), (0, 1, 0)))
    light = b.add_emitter((5.0, 5.0, 5.0))
    for k in range(17):
        b.add_instance(quad, light, translate((3.0 * k, 0, 0)))
    out.append(("emitters17", b.build(), None))
    # emissive spheres beside emissive triangle instances: the table counts triangle instances only, so 16 + 2 still has one
    # (of 16 entries) and 14 + 1 has 14; a scene with a sphere renders through an instantiation that never consults the table,
    # so only the host side can show this rule
    for lamps, spheres in ((16, 2), (14, 1)):
        b = SceneBuilder("emitters%d_spheres%d" % (lamps, spheres))
        quad = b.add_mesh(*scenes._quad((-1, 0, 1), (1, 0, 1), (1, 0, -1), (-1, 0, -1), (0, 1, 0)))
        light = b.add_emitter((5.0, 5.0, 5.0))
        for k in range(lamps):
            if k == spheres:  # (spheres between the triangle instances, not behind them all)
                for j in range(spheres):
                    b.add_sphere(light, 0.3, translate((3.0 * j, 4.0, 0)))
            b.add_instance(quad, light, translate((3.0 * k, 0, 0)))
        out.append(("emitters%d_spheres%d" % (lamps, spheres), b.build(), None))
    # two grids back to back
    sc = foggy_cornell()[0]
    sc.volumes = [sc.volumes[0], sc.volumes[0].copy()]
    out.append(("two_grids", sc, None))
    return out


def test_scene_prepare_matches_its_numpy_restatement(scene_prepare_check, tmp_path):
    """analyse_materials, layout_images, layout_alpha_masks, emitter_bounds and volume_first_words against the float32
    restatement above, byte for byte, under ASan + UBSan."""
    for name, sc, has_specular in _prepared_scenes():
        d = _dump_arrays(tmp_path / name, sc)
        results = _expect(d, sc)
        if has_specular is not None:
            assert results["scene_flags"][0] == has_specular, name
        if name == "mip_chains_and_masks":
            assert results["image_table"]["levels"][9] == 16 and results["image_table"]["w"][9][15] == 1  # 65535 x 1
            assert [int(t["levels"]) for t in results["image_table"][[0, 2, 3]]] == [1, 2, 3]  # 1x1, 2x2, 3x5
        if name == "emitters17":
            assert results["emitter_count"] == 0
        if name in ("emitters16_spheres2", "emitters14_spheres1"):
            assert results["emitter_count"] == int(name[8:10]) and sc.light_count == int(name[8:10]) + int(name[-1])
        if name == "cornell_box":
            assert results["emitter_count"] == 1 and results["emitters"]["identity"][0] == 1
        if name == "shared_mesh_scene":
            assert results["emitter_count"] == 1 and results["emitters"]["identity"][0] == 0
        if name == "two_grids":
            assert list(results["volume_first_words"]) == [0, sc.volumes[0].nbytes // 4]
        out = _run_prepare(scene_prepare_check, "results", d)
        assert "SCENE PREPARE OK" in out and out.count("bytes agree") == len(results), name + ": " + out
