"""The C++ host (stratum_amd/host/stratum_hip.hpp) changes only the environment of a scene between two frames:
Environment::set_value / mark_image_dirty, Scene::update, and BDPT::update must send the change through
sthip_scene_set_environment instead of an upload (tests/cpp/environment_host.cpp)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from stratum_amd import camera  # noqa: E402
from test_environment import CAM, RENDER_A, RENDER_B, sky_scene  # noqa: E402

ENVIRONMENT_HOST = os.path.join(ROOT, "tests", "cpp", "environment_host")
VALUE = (0.5, 1.25, 2.0)  # what the program sets


@pytest.fixture(scope="module")
def environment_host(built):
    src = os.path.join(ROOT, "tests", "cpp", "environment_host.cpp")
    deps = [src, os.path.join(ROOT, "tests", "cpp", "scene_reader.hpp"), os.path.join(ROOT, "stratum_amd", "host", "stratum_hip.hpp"), os.path.join(ROOT, "include", "sthip.h")]
    if not os.path.exists(ENVIRONMENT_HOST) or os.path.getmtime(ENVIRONMENT_HOST) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(
            ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-o", ENVIRONMENT_HOST, src, "-L" + os.path.join(ROOT, "stratum_amd"), "-lstratum_hip", "-Wl,-rpath," + os.path.join(ROOT, "stratum_amd")]
        )
    return ENVIRONMENT_HOST


def test_cpp_host_with_environment_hooks_builds(environment_host):
    """Environment::set_value / mark_image_dirty, make_environment(..., tables_on_device) and BDPT::update's environment-only
    path compile and link against the library (no GPU needed); without arguments the program only prints its usage."""
    out = subprocess.run([environment_host], capture_output=True, text=True)
    assert out.returncode == 2 and "usage: environment_host" in out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("mode,share,report", [
    ((), False, "environment_only=1 uploads=1 environment_calls=1 same_as_from_start=1 fresh_uploads=1 fresh_environment_calls=1"),
    (("--device-tables",), False, "environment_only=1 uploads=1 environment_calls=2 same_as_from_start=1 fresh_uploads=1 fresh_environment_calls=1"),
    # without the symbol (Scene::set_environment_on_device(false)): the same program uploads and passes
    (("--host-only",), False, "environment_only=0 uploads=2 environment_calls=0 same_as_from_start=1 fresh_uploads=1 fresh_environment_calls=0"),
    # the environment is not the only change (an instance moves in the same frame): the changed sky arrives by an upload,
    # whether its tables are the host's (stale after mark_image_dirty: the device builds them behind the upload) or the device's
    (("--move",), False, "environment_only=0 uploads=2 environment_calls=1 same_as_from_start=1 fresh_uploads=1 fresh_environment_calls=1"),
    (("--device-tables", "--move"), False, "environment_only=0 uploads=2 environment_calls=2 same_as_from_start=1 fresh_uploads=1 fresh_environment_calls=1"),
    (("--host-only", "--move"), False, "environment_only=0 uploads=2 environment_calls=0 same_as_from_start=1 fresh_uploads=1 fresh_environment_calls=0"),
    # a material shares the environment's image: the library refuses the call as unsupported (one attempt), the host uploads
    # and the device builds the tables behind each upload
    (("--device-tables",), True, "environment_only=0 uploads=2 environment_calls=3 same_as_from_start=1 fresh_uploads=1 fresh_environment_calls=1"),
    ((), True, "environment_only=0 uploads=2 environment_calls=2 same_as_from_start=1 fresh_uploads=1 fresh_environment_calls=1"),
])
def test_gpu_cpp_host_changes_only_the_environment(environment_host, tmp_path, mode, share, report):
    from stratum_amd.bdpt import BDPT
    from stratum_amd.scene import dump_description

    W, H, seeds = 48, 32, 2
    fr = camera.Frame(W, H, CAM["fovy"], CAM["eye"], CAM["target"])
    sc = sky_scene(RENDER_A, share=share)
    moved = "--move" in mode
    desc, sky, outp = str(tmp_path / "scene.bin"), str(tmp_path / "sky.bin"), str(tmp_path / "out.bin")
    dump_description(desc, sc, fr)
    with open(sky, "wb") as f:
        f.write(np.array(RENDER_B.shape[:2], np.uint32).tobytes())
        f.write(np.ascontiguousarray(RENDER_B, np.float32).tobytes())
    out = subprocess.run([environment_host, *mode, desc, sky, outp, str(seeds)], capture_output=True, text=True)
    assert out.returncode == 0 and ("ENVIRONMENT " + report) in out.stdout, out.stdout + out.stderr
    raw = np.fromfile(outp, dtype=np.uint8)
    rad = raw[: W * H * 16].view(np.float32).reshape(H, W, 4)
    prev_uv = raw[W * H * 16 : W * H * 24].view(np.float32).reshape(H, W, 2)
    rays = raw[W * H * 24 : W * H * 24 + 16].view(np.uint64)
    r = BDPT(device=0)
    try:
        r.update(sc)
        first = np.array(r.render(fr, 0, seeds)["radiance"], copy=True)
        if share or moved:  # what the C++ host had to do as well: the scene with the new environment (and the move) goes up again
            sc = sky_scene(RENDER_B, VALUE, share=share)
            if moved:
                from stratum_amd.scene import translate

                f32 = np.float32  # (the program adds in binary32 to the node's binary32 translation)
                sc.set_instance_transform(1, translate((float(f32(0.0) + f32(0.25)), float(f32(1.8) + f32(0.125)), float(f32(0.0) - f32(0.25)))))
            r.update(sc)
        else:
            r.set_environment(value=VALUE, image=RENDER_B)
        ref = r.render(fr, seeds, seeds)  # the C++ host's frame number went on: seeds `seeds` .. 2 seeds - 1
        assert np.array_equal(rad.view(np.uint32), ref["radiance"].view(np.uint32))
        assert np.array_equal(prev_uv.view(np.uint32), ref["prev_uv"].view(np.uint32))
        assert np.array_equal(rays, ref["ray_count"])
        assert not np.array_equal(first, ref["radiance"])
    finally:
        r.close()
