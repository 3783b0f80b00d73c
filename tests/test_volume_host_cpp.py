"""The C++ host (stratum_amd/host/stratum_hip.hpp): a Medium whose density comes from a dense box in device memory
(Medium::set_density_device) and whose grid is the only change of a frame is sthip_scene_set_volume instead of an upload
(tests/cpp/volume_host.cpp)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import volume_cases as vc  # noqa: E402
from stratum_amd import camera, scenes  # noqa: E402

VOLUME_HOST = os.path.join(ROOT, "tests", "cpp", "volume_host")


@pytest.fixture(scope="module")
def volume_host(built):
    src = os.path.join(ROOT, "tests", "cpp", "volume_host.cpp")
    deps = [src, os.path.join(ROOT, "tests", "cpp", "scene_reader.hpp"), os.path.join(ROOT, "stratum_amd", "host", "stratum_hip.hpp"), os.path.join(ROOT, "include", "sthip.h")]
    if not os.path.exists(VOLUME_HOST) or os.path.getmtime(VOLUME_HOST) < max(os.path.getmtime(d) for d in deps):
        rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
        subprocess.check_call(
            [os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", VOLUME_HOST, src,
             "-L" + os.path.join(ROOT, "stratum_amd"), "-lstratum_hip", "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "stratum_amd"), "-Wl,-rpath," + os.path.join(rocm, "lib")]
        )
    return VOLUME_HOST


def test_cpp_host_with_volume_hooks_builds(volume_host):
    """Medium::set_density_device, the volumes-only branch of BDPT::update and its fallback compile and link against the library
    (no GPU needed); without arguments the program only prints its usage."""
    out = subprocess.run([volume_host], capture_output=True, text=True)
    assert out.returncode == 2 and "usage: volume_host" in out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("mode,report", [
    # the grid is the only change: one call, no second upload; the graph that has the source from the start builds it for its upload
    ((), "volumes_only=1 uploads=1 volume_calls=1 same_as_from_start=1 fresh_uploads=1 fresh_volume_calls=0"),
    # without the call (BDPT::set_volumes_on_device(false)): the grid is built into the host's buffer and the scene goes up again
    (("--host-only",), "volumes_only=0 uploads=2 volume_calls=0 same_as_from_start=1 fresh_uploads=1 fresh_volume_calls=0"),
])
def test_gpu_cpp_host_changes_only_the_volume(volume_host, tmp_path, mode, report):
    from stratum_amd.bdpt import BDPT
    from stratum_amd.scene import dump_description

    W, H, seeds = 48, 32, 2
    dense, origin, _, _, nm = vc.case("cropped")
    voxel, tr = 0.05, (0.0, -0.4, -205.0)  # (into the Cornell box: the case's origin lies at z = 4090)
    sc, cam = scenes.cornell_box(fog=vc.fixture()["grid"])
    fr = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
    desc, dense_path, outp = str(tmp_path / "scene.bin"), str(tmp_path / "dense.bin"), str(tmp_path / "out.bin")
    dump_description(desc, sc, fr)
    with open(dense_path, "wb") as f:
        f.write(np.array(dense.shape, np.uint32).tobytes() + np.array(origin, np.int32).tobytes() + np.array([voxel, *tr], np.float64).tobytes() + np.ascontiguousarray(dense, np.float32).tobytes())
    out = subprocess.run([volume_host, *mode, desc, dense_path, outp, str(seeds)], capture_output=True, text=True)
    assert out.returncode == 0 and ("VOLUME " + report) in out.stdout, out.stdout + out.stderr
    raw = np.fromfile(outp, dtype=np.uint8)
    rad = raw[: W * H * 16].view(np.float32).reshape(H, W, 4)
    prev_uv = raw[W * H * 16 : W * H * 24].view(np.float32).reshape(H, W, 2)
    rays = raw[W * H * 24 : W * H * 24 + 16].view(np.uint64)
    r = BDPT(device=0)
    try:
        r.update(sc)
        first = np.array(r.render(fr, 0, seeds)["radiance"], copy=True)
        r.set_volume(0, dense=np.array(dense), origin=origin, voxel_size=voxel, translation=tr, name="density")
        ref = r.render(fr, seeds, seeds)  # the C++ host's frame number went on: seeds `seeds` .. 2 seeds - 1
        assert np.array_equal(rad.view(np.uint32), ref["radiance"].view(np.uint32))
        assert np.array_equal(prev_uv.view(np.uint32), ref["prev_uv"].view(np.uint32))
        assert np.array_equal(rays, ref["ray_count"])
        assert not np.array_equal(first, ref["radiance"])
    finally:
        r.close()
