"""sthip_scene_set_images / sthip_scene_set_material_data / sthip_scene_read_image_range (include/sthip.h: "the materials of a
resident scene"): texels and record bytes replaced in a resident scene, the mip chains and the image ranges made again on the
device, the material analysis made again on the host.

The reference of the range kernel is numpy's nanmin / nanmax with the header's NaN rule, pinned by tests/cpp/image_range_ref.cpp
(a scalar C++ restatement written from the header's text). The reference of every frame is a fresh context that uploaded the
edited scene, and the CPU oracle."""
import copy
import ctypes as C
import functools
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from stratum_amd import camera, scenes, wire  # noqa: E402
from stratum_amd.scene import SceneBuilder, translate  # noqa: E402

F32 = np.float32
OUTPUTS = ("radiance", "albedo", "visibility", "depth", "prev_uv", "ray_count")
CXX = os.environ.get("CXX", "g++")
REF_SRC = os.path.join(ROOT, "tests", "cpp", "image_range_ref.cpp")
CHECK_SRC = os.path.join(ROOT, "tests", "cpp", "material_update_check.cpp")
SYMBOLS = ("sthip_scene_set_images", "sthip_scene_set_material_data", "sthip_scene_read_image_range")


# ---------------------------------------------------------------------------------------------------------------------------
# image ranges: the cases and their numpy reference
# ---------------------------------------------------------------------------------------------------------------------------
EXTENTS = [(1, 1), (3, 1), (8, 8), (13, 5), (64, 65), (257, 129)]  # (W, H): 1, 3, 64, 65 texels; 65 waves; more than a block per trip


def np_range(img):
    """(lo[4], hi[4], nan_mask) of an (H, W, 4) float32 or uint8 image by the rule of include/sthip.h."""
    flat = img.reshape(-1, 4)
    if img.dtype == np.uint8:
        return (flat.min(0).astype(F32) / F32(255)).astype(F32), (flat.max(0).astype(F32) / F32(255)).astype(F32), 0
    nan = np.isnan(flat).any(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (an all-NaN channel)
        lo, hi = np.nanmin(flat, 0).astype(F32), np.nanmax(flat, 0).astype(F32)
    lo[nan], hi[nan] = -np.inf, np.inf
    return lo, hi, int(sum(1 << c for c in range(4) if nan[c]))


def planted_positions(n):
    """Flat texel indices where an extreme can be lost: the first and the last texel, the last lane of a full wave (one RGBA32F
    texel per lane: 63; four RGBA8 texels per lane: 252 .. 255), the first texel of the tail behind the last full wave, and the
    texels around the last 16-byte boundary of an RGBA8 image."""
    want = [0, n - 1, 63, 64, 252, 255, 256, (n // 64) * 64, (n // 256) * 256, (n // 4) * 4, n - 2, n - 3, n - 4, 1, 2, 3]
    return sorted({p for p in want if 0 <= p < n})


def base_image(w, h, dtype, seed):
    rng = np.random.RandomState(seed)
    if dtype == np.uint8:
        return rng.randint(60, 200, size=(h, w, 4)).astype(np.uint8)
    return rng.uniform(0.25, 0.75, size=(h, w, 4)).astype(F32)


def range_cases(w, h, dtype):
    """name -> image. Every planted position holds, in its own variant, the minimum of one channel and the maximum of another;
    float images also get a NaN in one channel only, both infinities, denormal minima of both signs, zeros of both signs, and a
    channel of nothing but NaNs."""
    n = w * h
    out = {}
    lo_value, hi_value = (np.uint8(3), np.uint8(250)) if dtype == np.uint8 else (F32(-7.5), F32(9.25))
    for k, p in enumerate(planted_positions(n)):
        img = base_image(w, h, dtype, 11 + k)
        img.reshape(-1, 4)[p, k % 4] = lo_value
        img.reshape(-1, 4)[p, (k + 1) % 4] = hi_value
        out["extremes_at_%d" % p] = img
    if dtype == np.uint8:
        img = base_image(w, h, dtype, 5)
        img.reshape(-1, 4)[n // 2] = (0, 255, 0, 255)
        out["bytes_0_and_255"] = img
        return out
    specials = {
        "nan_in_one_channel": [(n // 2, 2, np.nan)],
        "infinities": [(0, 0, np.inf), (n - 1, 1, -np.inf)],
        "denormal_minimum": [(n // 3, 0, 1e-41), (n // 2, 1, -1e-41), (n - 1, 2, 1e-45)],
        "zeros_of_both_signs": [(0, 0, 0.0), (n - 1, 0, -0.0), (n // 2, 1, -0.0)],
        "nan_and_extremes": [(0, 3, np.nan), (n - 1, 3, -100.0), (n // 2, 0, 50.0), (n // 2, 1, np.inf)],
    }
    for name, plants in specials.items():
        img = base_image(w, h, dtype, 7)
        for p, c, v in plants:
            img.reshape(-1, 4)[p, c] = F32(v)
        out[name] = img
    img = base_image(w, h, dtype, 9)
    img[..., 1] = np.nan
    out["all_nan_channel"] = img
    return out


def run_range_ref(exe, tmp, img):
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([1 if img.dtype == np.uint8 else 0, img.shape[0] * img.shape[1]], np.uint32).tobytes())
        f.write(np.ascontiguousarray(img).tobytes())
    subprocess.check_call([exe, fin, fout])
    raw = np.fromfile(fout, np.uint32)
    return raw[:4].view(F32), raw[4:8].view(F32), int(raw[8])


def same_range(got, want):
    """Value for value (-0 == +0, an infinity equals itself), and the NaN mask."""
    return bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2] and not np.isnan(got[0]).any() and not np.isnan(got[1]).any())


# ---------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_library_exports_and_header_declares_the_symbols(built):
    from stratum_amd import _lib

    L = _lib.lib()
    hdr_text = open(os.path.join(ROOT, "include", "sthip.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
        assert re.search(r"^int %s\(sthip_ctx\*" % name, hdr_text, re.M), name
    assert L.sthip_abi_version() == 11 and "#define STHIP_ABI_VERSION 11" in hdr_text
    for phrase in ("typedef struct sthip_image_update", "the sign of a zero result is NOT part of the contract", "(float)b / 255.0f", '"image_range_blocks"',
                   "A library without the feature lacks the three symbols"):
        assert phrase in hdr_text, phrase
    assert C.sizeof(wire.ImageUpdate) == 32 and C.sizeof(wire.ImagesInfo) == 24


def test_cpp_restatement_equals_numpy(tmp_path):
    exe = str(tmp_path / "image_range_ref")
    subprocess.check_call([CXX, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-o", exe, REF_SRC])
    count = 0
    for w, h in EXTENTS[:5]:
        for dtype in (F32, np.uint8):
            for name, img in range_cases(w, h, dtype).items():
                assert same_range(run_range_ref(exe, str(tmp_path), img), np_range(img)), (w, h, dtype, name)
                count += 1
    assert count > 100
    # the cases do what they are planted for
    lo, hi, mask = np_range(range_cases(13, 5, F32)["nan_in_one_channel"])
    assert mask == 4 and lo[2] == -np.inf and hi[2] == np.inf and np.isfinite(lo[[0, 1, 3]]).all()
    lo, hi, mask = np_range(range_cases(13, 5, F32)["all_nan_channel"])
    assert mask == 2 and lo[1] == -np.inf and hi[1] == np.inf
    lo, hi, mask = np_range(range_cases(13, 5, F32)["denormal_minimum"])
    assert mask == 0 and lo[0] == F32(1e-41) and lo[1] == F32(-1e-41) and 0 < lo[2] < np.finfo(F32).tiny
    lo, hi, mask = np_range(range_cases(13, 5, F32)["infinities"])
    assert hi[0] == np.inf and lo[1] == -np.inf and mask == 0


def test_host_checks_and_split_analysis_under_sanitizers(tmp_path):
    """tests/cpp/material_update_check.cpp links scene_prepare.cpp only: every refusal of both calls returns its code and message,
    and the analysis with supplied ranges equals analyse_materials on the same scene, under -fsanitize=address,undefined."""
    exe = str(tmp_path / "material_update_check")
    san = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall"]
    subprocess.check_call([CXX] + san + ["-o", exe, CHECK_SRC, os.path.join(ROOT, "stratum_amd", "csrc", "scene_prepare.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "MATERIAL UPDATE CHECK OK" in out.stdout and "FAIL" not in out.stdout, out.stdout + out.stderr
    for case in ("float image, mirror", "8-bit image, mirror", "image with a NaN", "constant without a positive component", "no scene", "struct_size", "which out of range",
                 "image index out of range", "NULL pixels", "differing extent", "the same image twice", "RGBA32F device pointer off 16 bytes", "RGBA8 device pointer off 4 bytes",
                 "a colour edit", "a triangle instance loses its mask", "a medium's volume changes", "a light goes out", "a surface starts to emit"):
        assert re.search(r"^ok\s+%s" % re.escape(case), out.stdout, re.M), case
    ref = str(tmp_path / "image_range_ref_san")
    subprocess.check_call([CXX] + san + ["-o", ref, REF_SRC])
    for name in ("extremes_at_0", "nan_in_one_channel", "all_nan_channel"):
        img = range_cases(13, 5, F32)[name]
        assert same_range(run_range_ref(ref, str(tmp_path), img), np_range(img)), name


def test_cpp_host_takes_the_material_branch_over_stand_ins(tmp_path):
    """tests/cpp/material_host.cpp: BDPT::update of stratum_hip.hpp over stand-ins for the C ABI (no GPU; the stand-ins refuse with
    the library's own host checks). A colour edit is one sthip_scene_set_material_data of the differing bytes, a repainted texture
    one sthip_scene_set_images, neither uploads; a changed extent, an emitter that goes out and a driver with the branch switched
    off (what MultiDeviceBDPT does) upload."""
    from stratum_amd.scene import dump_description

    exe, desc = str(tmp_path / "material_host"), str(tmp_path / "scene.bin")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "cpp", "material_host.cpp"),
                           os.path.join(ROOT, "stratum_amd", "csrc", "scene_prepare.cpp")])
    sc, cam = scenes.textured_box()
    dump_description(desc, sc, camera.Frame(16, 8, cam["fovy"], cam["eye"], cam["target"]))
    want = {
        "colour": dict(materials_only=1, uploads=1, data_calls=1, image_calls=0, data_bytes=4, images_sent=0),
        "texture": dict(materials_only=1, uploads=1, data_calls=0, image_calls=1, images_sent=1),
        "both": dict(materials_only=1, uploads=1, data_calls=1, image_calls=1, data_bytes=4, images_sent=1),
        "extent": dict(materials_only=0, uploads=2, data_calls=0, image_calls=0),
        "emitter": dict(materials_only=0, uploads=2, image_calls=0),
        "off": dict(materials_only=0, uploads=2, data_calls=0, image_calls=0),
    }
    for mode, fields in want.items():
        out = subprocess.run([exe, desc, mode], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.startswith("MATERIALS mode=%s " % mode), out.stdout + out.stderr
        got = dict(kv.split("=") for kv in out.stdout.split()[1:])
        for k, v in fields.items():
            assert int(got[k]) == v, (mode, k, out.stdout)
        assert got["refused"] == "0" and got["host_data_calls"] == got["data_calls"] and got["host_image_calls"] == got["image_calls"], out.stdout
    assert "mMaterialsOnDevice = false" in open(os.path.join(ROOT, "stratum_amd", "host", "stratum_hip_multi.hpp")).read()


# ---------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------
def decode(img):
    return (img.astype(F32) / F32(255)).astype(F32)


def one_image_scene(img):
    """A lit quad whose material binds `img` as its parameter image (metallic, roughness): the analysis reads its range. A 1 x 1
    image of the same format comes first in gImages, so that an RGBA8 `img` starts one word off a 16-byte boundary."""
    b = SceneBuilder("one_image")
    first = b.add_image(np.full((1, 1, 4), 200, np.uint8) if img.dtype == np.uint8 else np.full((1, 1, 4), 0.5, F32))
    floor = b.add_material((0.6, 0.6, 0.6), roughness=0.7)
    b.set_material_images(floor, base_color_image=first)
    quad = b.add_material((0.8, 0.8, 0.8), metallic=1.0, roughness=1.0)
    b.set_material_images(quad, params_image=b.add_image(img))
    lamp = b.add_emitter((9.0, 7.0, 5.0))
    b.add_instance(b.add_mesh(*scenes._quad((-3, 0, 3), (3, 0, 3), (3, 0, -3), (-3, 0, -3), (0, 1, 0))), floor)
    b.add_instance(b.add_mesh(*scenes._quad((-1, 0.5, 1), (1, 0.5, 1), (1, 0.5, -1), (-1, 0.5, -1), (0, 1, 0))), quad, translate((0.0, 0.1, 0.0)))
    b.add_instance(b.add_mesh(*scenes._quad((-0.4, 0, -0.4), (0.4, 0, -0.4), (0.4, 0, 0.4), (-0.4, 0, 0.4), (0, -1, 0))), lamp, translate((0.0, 1.8, 0.0)))
    return b.build()


SIZES = [(16, 16), (3, 5), (7, 1), (16, 16), (1, 1)]  # (H, W) of the five images of textured_box, in gImages order; 3 is the metal ball's parameter image


@functools.lru_cache(maxsize=None)
def _textured():
    return scenes.textured_box(mirror_map=False)


def params_bytes(mirror, seed=3):
    """The metal ball's parameter image (R scales metallic = 1, G scales roughness = 0.6) as bytes: rough everywhere, or with a
    checker of G = 0 texels, where the ball is a mirror by the texels alone."""
    rng = np.random.RandomState(seed)
    img = np.zeros((16, 16, 4), np.uint8)
    img[..., 0] = 255
    img[..., 1] = rng.randint(120, 256, size=(16, 16))
    img[..., 3] = 255
    if mirror:
        yy, xx = np.mgrid[0:16, 0:16]
        img[..., 1][((yy // 4 + xx // 4) % 2) == 0] = 0
    return img


def box_scene(as_bytes, mirror, seed=3):
    """textured_box with small random images, all RGBA8 or all RGBA32F (the same texels: bytes / 255)."""
    base, cam = _textured()
    sc = copy.copy(base)
    sc.materials = base.materials.copy()
    rng = np.random.RandomState(40)
    images = [rng.randint(0, 256, size=(h, w, 4)).astype(np.uint8) for h, w in SIZES]
    images[3] = params_bytes(mirror, seed)
    assert len(base.images) == 5
    sc.images = [np.ascontiguousarray(i if as_bytes else decode(i)) for i in images]
    return sc, cam


def sky_image():
    rng = np.random.RandomState(31)
    image = np.ones((16, 32, 4), F32)
    image[..., :3] = rng.uniform(0.1, 1.0, size=(16, 32, 3))
    return image


def sky_scene(share, image=None):
    """An emissive quad over a diffuse floor under an image environment. share: the floor's base colour binds the environment's
    image; otherwise no material record binds an image."""
    image = sky_image() if image is None else image
    b = SceneBuilder("sky")
    floor = b.add_material((0.6, 0.6, 0.6), roughness=0.7)
    lamp = b.add_emitter((9.0, 7.0, 5.0))
    handle = b.add_image(image)
    if share:
        b.set_material_images(floor, base_color_image=handle)
    b.add_instance(b.add_mesh(*scenes._quad((-3, 0, 3), (3, 0, 3), (3, 0, -3), (-3, 0, -3), (0, 1, 0))), floor)
    b.add_instance(b.add_mesh(*scenes._quad((-0.4, 0, -0.4), (0.4, 0, -0.4), (0.4, 0, 0.4), (-0.4, 0, 0.4), (0, -1, 0))), lamp, translate((0.0, 1.8, 0.0)))
    b.set_environment((1.0, 1.0, 1.0), handle)
    return b.build(), {"eye": (0.0, 1.2, 5.0), "target": (0.0, 0.7, 0.0), "fovy": np.radians(45.0)}


def record_address(sc, base_color):
    """Byte address of the material record whose base colour is `base_color`."""
    recs = sc.materials[: (sc.materials.size // 72) * 72].reshape(-1, 72)
    want = np.array(base_color, F32).view(np.uint8)
    hits = [k * 72 for k, r in enumerate(recs) if np.array_equal(r[:12], want)]
    assert len(hits) == 1, hits
    return hits[0]


def edited(sc, edits):
    out = copy.copy(sc)
    out.materials = sc.materials.copy()
    for offset, data in edits:
        b = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        out.materials[offset : offset + b.size] = b
    return out


ARGS = {"maxPathVertices": 6, "maxDiffuseVertices": 2}  # the diffuse budget ends paths early unless some material can be specular


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def make_renderer(flags=(), args=None, options=None):
    from stratum_amd.bdpt import BDPT

    r = BDPT(device=0, args=dict(ARGS if args is None else args, bdptFlag=list(flags)))
    for k, v in (options or {}).items():
        r.set_option(k, v)
    return r


def frame_copy(out):
    return {k: np.array(v, copy=True) for k, v in out.items() if isinstance(v, np.ndarray)}


def same_frame(got, want, what):
    for k in OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), (what, k)


def frame_of(cam):
    return camera.Frame(48, 32, cam["fovy"], cam["eye"], cam["target"])


def fresh_frame(sc, cam, flags, options=None, seeds=2, seed_begin=0):
    r = make_renderer(flags, options=options)
    try:
        r.update(sc)
        return frame_copy(r.render(frame_of(cam), seed_begin, seeds))
    finally:
        r.close()


def decoded(sc):
    """`sc` with its 8-bit images as float images bytes / 255: the scene the oracle reads (without ray cones an RGBA8 frame is that
    scene's frame, and an R8 mask gives the float mask's: tests/test_image_formats.py)."""
    out = copy.copy(sc)
    out.images = [decode(i) if i.dtype == np.uint8 else i for i in sc.images]
    out.images1 = [decode(i) if i.dtype == np.uint8 else i for i in sc.images1]
    return out


def against_the_oracle(r, got, sc, cam, what, seeds=2, seed_begin=0):
    """The radiance and the ray count of the CPU oracle for `sc` (a float scene), bit for bit."""
    from oracle import oracle_py

    frame = frame_of(cam)
    ref = oracle_py.OracleScene(sc).render(frame, r.push_constants(frame), r.mSamplingFlags, seed_begin, seeds)
    differing = int((got["radiance"].view(np.uint32) != np.ascontiguousarray(ref["radiance"]).view(np.uint32)).any(axis=-1).sum())
    print("%s: %d of %d radiance pixels differ from the oracle" % (what, differing, 48 * 32))
    assert np.array_equal(got["radiance"].view(np.uint8), np.ascontiguousarray(ref["radiance"]).view(np.uint8)), what
    assert np.array_equal(got["ray_count"], ref["ray_count"]), what


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [1, 3, 0], ids=["one_block", "three_blocks", "default_grid"])
@pytest.mark.parametrize("dtype", [F32, np.uint8], ids=["rgba32f", "rgba8"])
def test_gpu_range_kernel_equals_the_restatement(built, dtype, blocks):
    """k_image_range through sthip_scene_read_image_range, value for value against the numpy statement that
    tests/cpp/image_range_ref.cpp pins: every extent, every planted position and special value, with one block (every texel in
    one grid-stride loop: the second trip at 8 x 8 and beyond), three blocks (more blocks than texels at 1 x 1) and the default."""
    r = make_renderer(options={"image_range_blocks": blocks})
    try:
        for w, h in EXTENTS:
            cases = range_cases(w, h, dtype)
            r.update(one_image_scene(base_image(w, h, dtype, 1)))
            assert same_range(r.read_image_range(1), np_range(base_image(w, h, dtype, 1))), (w, h, "the upload's host scan")
            for name, img in cases.items():
                info = r.set_images({1: img})
                assert info["images_scanned"] == 1, (w, h, name)
                got, want = r.read_image_range(1), np_range(img)
                assert same_range(got, want), (w, h, name, got, want)
            assert np.array_equal(np.ascontiguousarray(r.read_image(1, 0)).view(np.uint8), img.view(np.uint8))
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_range_from_a_device_pointer_and_several_images_in_one_call(built):
    import torch

    r = make_renderer()
    try:
        sc, _ = box_scene(as_bytes=False, mirror=False)
        r.update(sc)
        new = {k: np.ascontiguousarray(base_image(w, h, F32, 80 + k)) for k, (h, w) in enumerate(SIZES)}
        new[2][3, 0, 1] = np.nan
        dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in new.items()}
        torch.cuda.synchronize()
        info = r.set_images(dev, device_ptr=True)
        assert info["images_scanned"] == 5
        for k, v in new.items():
            assert np.array_equal(r.read_image(k, 0).view(np.uint32), v.view(np.uint32)), k
        assert same_range(r.read_image_range(3), np_range(new[3]))  # (the image the analysis reads; the others are named under base colours and a bump map)
        assert r.read_image_range(2)[2] == 2
        from stratum_amd import _lib

        r.update(sky_scene(share=False)[0])
        with pytest.raises(_lib.StratumHipError, match=r"\(-1\).*holds no range"):
            r.read_image_range(0)  # (the environment's image: no material names it)
        with pytest.raises(_lib.StratumHipError, match=r"\(-1\).*not in gImages"):
            r.read_image_range(1)
        for bad in (-1, 65536):
            with pytest.raises(_lib.StratumHipError, match="image_range_blocks"):
                r.set_option("image_range_blocks", bad)
    finally:
        r.close()


def float_chain(img):
    levels, cur = [], np.asarray(img, F32)
    while cur.shape[0] > 1 or cur.shape[1] > 1:
        h, w = cur.shape[:2]
        nh, nw = max(1, h // 2), max(1, w // 2)
        y0, y1 = np.minimum(2 * np.arange(nh), h - 1), np.minimum(2 * np.arange(nh) + 1, h - 1)
        x0, x1 = np.minimum(2 * np.arange(nw), w - 1), np.minimum(2 * np.arange(nw) + 1, w - 1)
        a, b, c, e = cur[y0][:, x0], cur[y0][:, x1], cur[y1][:, x0], cur[y1][:, x1]
        cur = (((a + b) + (c + e)) * F32(0.25)).astype(F32)
        levels.append(cur)
    return levels


def byte_chain(img):
    levels, cur = [], np.asarray(img, np.uint8)
    while cur.shape[0] > 1 or cur.shape[1] > 1:
        h, w = cur.shape[:2]
        nh, nw = max(1, h // 2), max(1, w // 2)
        y0, y1 = np.minimum(2 * np.arange(nh), h - 1), np.minimum(2 * np.arange(nh) + 1, h - 1)
        x0, x1 = np.minimum(2 * np.arange(nw), w - 1), np.minimum(2 * np.arange(nw) + 1, w - 1)
        a, b, c, e = (cur[y][:, x].astype(np.uint32) for y, x in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
        cur = ((a + b + c + e + 2) >> 2).astype(np.uint8)
        levels.append(cur)
    return levels


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, np.uint8], ids=["rgba32f", "rgba8"])
def test_gpu_mip_chains_after_a_replacement(built, dtype):
    r = make_renderer()
    try:
        for w, h in ((5, 3), (7, 1), (1, 9)):
            r.update(one_image_scene(base_image(w, h, dtype, 1)))
            img = base_image(w, h, dtype, 2)
            r.set_images({1: img})
            chain = [img] + (byte_chain(img) if dtype == np.uint8 else float_chain(img))
            for level, want in enumerate(chain):
                got = r.read_image(1, level)
                assert got.dtype == want.dtype and got.shape == want.shape, (w, h, level)
                assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), (w, h, level)
    finally:
        r.close()


def params_after(as_bytes, mirror):
    img = params_bytes(mirror)
    return img if as_bytes else decode(img)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["rough_to_mirror", "mirror_to_rough", "rgba8_rough_to_mirror", "rgba8_light_tracing"])
def test_gpu_repainted_parameter_image(built, case):
    """The metal ball's roughness map is repainted. Rough to mirror: has_specular goes false to true, and with gMaxDiffuseVertices
    = 2 < gMaxPathVertices = 6 the frame under the old analysis would lose every path beyond the diffuse budget. Every output
    equals a fresh upload of the edited scene, and the oracle's radiance and ray count."""
    as_bytes = case.startswith("rgba8")
    to_mirror = case != "mirror_to_rough"
    flags = {"rough_to_mirror": ["~raycones"], "mirror_to_rough": [], "rgba8_rough_to_mirror": ["~raycones"], "rgba8_light_tracing": ["~raycones", "connecttoviews"]}[case]
    before_scene, cam = box_scene(as_bytes, mirror=not to_mirror)
    after_scene, _ = box_scene(as_bytes, mirror=to_mirror)
    frame = frame_of(cam)
    r = make_renderer(flags)
    try:
        r.update(before_scene)
        before = frame_copy(r.render(frame, 0, 2))
        info = r.set_images({3: params_after(as_bytes, to_mirror)})
        assert (info["has_specular_before"], info["has_specular_after"], info["images_scanned"]) == (int(not to_mirror), int(to_mirror), 1)
        assert info["device_ms"] >= 0 and info["total_ms"] > 0
        got = frame_copy(r.render(frame, 0, 2))
        same_frame(got, fresh_frame(after_scene, cam, flags), case)
        assert not np.array_equal(got["radiance"], before["radiance"])
        assert got["ray_count"][0] != before["ray_count"][0]  # (other paths: mirror texels take no shadow rays and run on past the diffuse budget)
        # (without ray cones level 0 alone is read, and an RGBA8 frame is the frame of the float scene bytes / 255: the oracle's scene)
        oracle_scene = box_scene(False, mirror=to_mirror)[0] if "~raycones" in flags else after_scene
        against_the_oracle(r, got, oracle_scene, cam, case)
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_constant_edit_of_an_untextured_scene(built):
    """Cornell box, no images: the red wall becomes a mirror (INST_FLAG_SPECULAR, has_specular false to true) and the green wall
    black (INST_FLAG_CAN_EVAL goes), the white colour changes: k_cull_terminal's table and the round counts follow. Under NEE."""
    sc, cam = scenes.cornell_box()
    red, green, white = (record_address(sc, c) for c in ((0.65, 0.05, 0.05), (0.12, 0.45, 0.15), (0.73, 0.73, 0.73)))
    edits = [(red + 20, np.array([1.0, 0.0], F32)), (green, np.array([0.0, 0.0, 0.0], F32)), (white, np.array([0.3, 0.5, 0.7], F32))]
    frame = frame_of(cam)
    flags = ["nee"]
    r = make_renderer(flags)
    try:
        r.update(edited(sc, []))
        before = frame_copy(r.render(frame, 0, 2))
        infos = [r.set_material_data(offset, data) for offset, data in edits]
        assert (infos[0]["has_specular_before"], infos[0]["has_specular_after"]) == (0, 1) and infos[2]["has_specular_after"] == 1
        assert all(i["images_scanned"] == 0 for i in infos)
        got = frame_copy(r.render(frame, 0, 2))
        want_scene = edited(sc, edits)
        same_frame(got, fresh_frame(want_scene, cam, flags), "constants")
        assert not np.array_equal(got["radiance"], before["radiance"]) and got["ray_count"][0] != before["ray_count"][0]
        against_the_oracle(r, got, want_scene, cam, "constants")
        # and back: the mirror becomes rough again
        info = r.set_material_data(red + 20, np.array([0.0, 0.5], F32))
        assert (info["has_specular_before"], info["has_specular_after"]) == (1, 0)
        same_frame(frame_copy(r.render(frame, 0, 2)), fresh_frame(edited(want_scene, [(red + 20, np.array([0.0, 0.5], F32))]), cam, flags), "constants, back")
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_a_record_starts_binding_an_image(built):
    """No record binds an image (the environment's image is the only one): k_shade runs untextured. The floor's base colour
    then binds image 0 and its parameters too: textured goes false to true, and the image, which nobody had scanned, is scanned
    on the device from its resident texels."""
    flags = ["~nee", "~sampleenvironmentmapdirectly"]
    sc, cam = sky_scene(share=False)
    want_scene, _ = sky_scene(share=True)
    floor = record_address(sc, (0.6, 0.6, 0.6))
    frame = frame_of(cam)
    r = make_renderer(flags)
    try:
        r.update(sc)
        before = frame_copy(r.render(frame, 0, 2))
        info = r.set_material_data(floor + 16, np.array([0], np.uint32))
        assert info["images_scanned"] == 0  # (a base colour's range is nobody's business)
        got = frame_copy(r.render(frame, 0, 2))
        same_frame(got, fresh_frame(want_scene, cam, flags), "binds an image")
        assert not np.array_equal(got["radiance"], before["radiance"])
        against_the_oracle(r, got, want_scene, cam, "binds an image")
        # the parameter value binds it too (metallic 1 under a texel range that reaches 1, roughness 0.7 * texel >= 0.07): scanned now
        params = np.zeros(5, np.uint32)
        params[:4] = np.array([1.0, 0.7, 0.0, 0.0], F32).view(np.uint32)
        info = r.set_material_data(floor + 20, params)
        assert info["images_scanned"] == 1 and info["has_specular_after"] == 0
        lo, hi, mask = r.read_image_range(0)
        assert same_range((lo, hi, mask), np_range(want_scene.images[0]))
        want2 = edited(want_scene, [(floor + 20, params)])
        same_frame(frame_copy(r.render(frame, 0, 2)), fresh_frame(want2, cam, flags), "binds the parameter image")
    finally:
        r.close()


NO_IMAGE = np.array([0xFFFFFFFF], np.uint32)


@pytest.mark.gpu
def test_gpu_unbind_repaint_rebind(built):
    """A range the context holds must be the resident texels'. The metal ball's parameter image is unbound (no record names it
    any more), repainted as a mirror while nobody names it (not scanned), and bound again: it is scanned then, has_specular goes
    true, and the frame is the fresh upload's and the oracle's. A range kept from the rough texels would end paths at the
    diffuse budget."""
    from stratum_amd import _lib

    flags = ["~raycones"]
    sc, cam = box_scene(False, mirror=False)
    want_scene, _ = box_scene(False, mirror=True)
    metal = record_address(sc, (0.9, 0.7, 0.4))
    frame = frame_of(cam)
    r = make_renderer(flags)
    try:
        r.update(sc)
        assert same_range(r.read_image_range(3), np_range(sc.images[3]))
        info = r.set_material_data(metal + 36, NO_IMAGE)
        assert info["images_scanned"] == 0 and info["has_specular_after"] == 0
        with pytest.raises(_lib.StratumHipError, match=r"\(-1\).*holds no range"):
            r.read_image_range(3)  # (no record names it any more)
        info = r.set_images({3: params_after(False, True)})
        assert info["images_scanned"] == 0 and info["has_specular_after"] == 0
        unbound = edited(want_scene, [(metal + 36, NO_IMAGE)])
        same_frame(frame_copy(r.render(frame, 0, 2)), fresh_frame(unbound, cam, flags), "unbound and repainted")
        info = r.set_material_data(metal + 36, np.array([3], np.uint32))
        assert (info["images_scanned"], info["has_specular_before"], info["has_specular_after"]) == (1, 0, 1)
        assert same_range(r.read_image_range(3), np_range(want_scene.images[3]))
        got = frame_copy(r.render(frame, 0, 2))
        same_frame(got, fresh_frame(want_scene, cam, flags), "bound again")
        against_the_oracle(r, got, want_scene, cam, "bound again")
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_environment_texels_replaced_while_unbound(built):
    """The same through sthip_scene_set_environment: the floor's parameters bind the environment's image (scanned: rough), the
    record lets go of it, the environment call replaces the texels (accepted now: no record names the image) with ones that make
    the floor a mirror somewhere, and the record binds the image again."""
    flags = ["~nee", "~sampleenvironmentmapdirectly"]
    sc, cam = sky_scene(share=False)
    mirror = sky_image()
    mirror[::2, ::2, 0] = 1.0  # metallic 1 * 1
    mirror[::2, ::2, 1] = 0.0  # roughness 0.7 * 0
    floor = record_address(sc, (0.6, 0.6, 0.6))
    params = np.zeros(5, np.uint32)
    params[:4] = np.array([1.0, 0.7, 0.0, 0.0], F32).view(np.uint32)
    frame = frame_of(cam)
    r = make_renderer(flags)
    try:
        r.update(sc)
        info = r.set_material_data(floor + 20, params)
        assert (info["images_scanned"], info["has_specular_after"]) == (1, 0)
        r.set_material_data(floor + 36, NO_IMAGE)
        r.set_environment(image=mirror)
        info = r.set_material_data(floor + 36, np.array([0], np.uint32))
        assert (info["images_scanned"], info["has_specular_before"], info["has_specular_after"]) == (1, 0, 1)
        assert same_range(r.read_image_range(0), np_range(mirror))
        want_scene = edited(sky_scene(share=False, image=mirror)[0], [(floor + 20, params)])
        got = frame_copy(r.render(frame, 0, 2))
        same_frame(got, fresh_frame(want_scene, cam, flags), "environment texels, bound again")
        against_the_oracle(r, got, want_scene, cam, "environment texels, bound again")
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_texels_from_convert_material_on_the_device(built):
    """sthip_convert_material in its device form leaves the three Disney images in device memory; sthip_scene_set_images takes
    the parameter image from there. The frame is the frame of a scene uploaded with the host form's output."""
    import torch

    from stratum_amd import _lib

    flags = ["~raycones"]
    sc, cam = box_scene(as_bytes=True, mirror=False)
    rng = np.random.RandomState(77)
    base = rng.randint(0, 256, size=(16, 16, 4)).astype(np.uint8)
    metal_rough = np.zeros((16, 16, 4), np.uint8)  # glTF: G = roughness, B = metallic
    metal_rough[..., 1] = params_bytes(True)[..., 1]
    metal_rough[..., 2] = 255
    metal_rough[..., 3] = 255
    r = make_renderer(flags)
    try:
        r.update(sc)
        host = r.convert_material("GltfPbr", diffuse=base, specular=metal_rough, output_format=1)
        d = wire.ConvertMaterialDesc()
        d.kind, d.width, d.height, d.device_ptrs, d.output_format = wire.CONVERT["GltfPbr"], 16, 16, 1, 1
        src = [torch.from_numpy(a).to("cuda:0") for a in (base, metal_rough)]
        d.gDiffuse, d.gSpecular, d.diffuse_format, d.specular_format = src[0].data_ptr(), src[1].data_ptr(), 1, 1
        outs = [torch.zeros((16, 16, 4), dtype=torch.uint8, device="cuda:0") for _ in range(3)]
        mask = torch.zeros((16, 16), dtype=torch.uint8, device="cuda:0")
        min_alpha = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        for k in range(3):
            d.gOutput[k] = outs[k].data_ptr()
        d.gOutputAlphaMask, d.gOutputMinAlpha = mask.data_ptr(), min_alpha.data_ptr()
        torch.cuda.synchronize()
        r._check(_lib.lib().sthip_convert_material(r._h, C.byref(d)), "sthip_convert_material")
        info = r.set_images({3: outs[1]}, device_ptr=True)  # (chained behind the conversion on the context's stream: no copy back)
        assert info["images_scanned"] == 1
        assert np.array_equal(r.read_image(3, 0), host["output"][1])
        assert same_range(r.read_image_range(3), np_range(host["output"][1]))
        want_scene = copy.copy(sc)
        want_scene.images = list(sc.images)
        want_scene.images[3] = host["output"][1]
        got = frame_copy(r.render(frame_of(cam), 0, 2))
        same_frame(got, fresh_frame(want_scene, cam, flags), "device pointer from convert_material")
        against_the_oracle(r, got, decoded(want_scene), cam, "device pointer from convert_material")
        # the scene object still holds the texels before; handed to update() again it first takes what is resident
        assert np.array_equal(sc.images[3], params_bytes(False))
        r.update(sc)
        assert np.array_equal(sc.images[3], host["output"][1])
        same_frame(frame_copy(r.render(frame_of(cam), 0, 2)), got, "the same scene object uploaded again")
    finally:
        r.close()


def foliage_scene(seed):
    base, cam = scenes.foliage()
    sc = copy.copy(base)
    rng = np.random.RandomState(seed)
    values = np.array([0, 64, 190, 191, 192, 193, 255], np.uint8)
    sc.images1 = [np.ascontiguousarray(rng.choice(values, size=(5, 7))), decode(np.ascontiguousarray(rng.choice(values, size=(7, 5))))]  # an R8 and an R32F mask
    return sc, cam


@pytest.mark.gpu
def test_gpu_replaced_alpha_masks(built):
    """Both masks of the foliage (one R8, one R32F) replaced under eAlphaTest: the frame of a fresh upload; kept first hits are
    dropped by a mask edit."""
    flags = ["alphatest"]
    sc, cam = foliage_scene(70)
    want_scene, _ = foliage_scene(71)
    frame = frame_of(cam)
    r = make_renderer(flags, options={"reuse_first_hits": 1})
    try:
        r.update(sc)
        before = frame_copy(r.render(frame, 0, 2))
        assert r.stats()["rays_primary_packets"] > 0
        r.render(frame, 0, 2)
        assert r.stats()["rays_primary_packets"] == 0
        info = r.set_images(masks={0: want_scene.images1[0], 1: want_scene.images1[1]})
        assert info["images_scanned"] == 0
        got = frame_copy(r.render(frame, 0, 2))
        assert r.stats()["rays_primary_packets"] > 0  # (the alpha test decides first hits)
        same_frame(got, fresh_frame(want_scene, cam, flags), "masks")
        assert not np.array_equal(got["visibility"]["instance_primitive_index"], before["visibility"]["instance_primitive_index"])
        oracle_scene = copy.copy(want_scene)  # (an R8 mask gives the frame of the float mask bytes / 255: tests/test_image_formats.py)
        oracle_scene.images1 = [decode(m) if m.dtype == np.uint8 else m for m in want_scene.images1]
        against_the_oracle(r, got, oracle_scene, cam, "masks")
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_kept_first_hits_survive_image_and_constant_edits(built):
    flags = ["~raycones"]
    sc, cam = box_scene(False, mirror=False)
    frame = frame_of(cam)
    wall = record_address(sc, (0.8, 0.75, 0.7))
    colour = np.array([0.2, 0.9, 0.4], F32)
    r = make_renderer(flags, options={"reuse_first_hits": 1})
    try:
        r.update(sc)
        r.render(frame, 0, 1)
        assert r.stats()["rays_primary_packets"] > 0
        r.set_images({3: params_after(False, True)})
        got = frame_copy(r.render(frame, 0, 1))
        assert r.stats()["rays_primary_packets"] == 0
        same_frame(got, fresh_frame(box_scene(False, mirror=True)[0], cam, flags, seeds=1), "kept first hits, image edit")
        against_the_oracle(r, got, box_scene(False, mirror=True)[0], cam, "kept first hits, image edit", seeds=1)
        r.set_material_data(wall, colour)
        got = frame_copy(r.render(frame, 0, 1))
        assert r.stats()["rays_primary_packets"] == 0
        same_frame(got, fresh_frame(edited(box_scene(False, mirror=True)[0], [(wall, colour)]), cam, flags, seeds=1), "kept first hits, constant edit")
        against_the_oracle(r, got, edited(box_scene(False, mirror=True)[0], [(wall, colour)]), cam, "kept first hits, constant edit", seeds=1)
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_persistent_reservoir_grids_restart(built):
    """reuse_grids_persist: the grids a call leaves carry the old materials' radiance; after an edit the next frame is a
    chain's first, as on a fresh context."""
    flags = ["neereservoirs", "neereservoirreuse"]
    options = {"reuse_grids_persist": 1}
    sc, cam = scenes.cornell_box()
    white = record_address(sc, (0.73, 0.73, 0.73))
    colour = np.array([0.3, 0.5, 0.7], F32)
    frame = frame_of(cam)
    r = make_renderer(flags, options=options)
    try:
        r.update(edited(sc, []))
        r.render(frame, 4, 1)
        chained = frame_copy(r.render(frame, 5, 1))
        r.set_material_data(white, colour)
        got = frame_copy(r.render(frame, 5, 1))
        first = fresh_frame(edited(sc, [(white, colour)]), cam, flags, options=options, seeds=1, seed_begin=5)
        same_frame(got, first, "the chain restarts")
        against_the_oracle(r, got, edited(sc, [(white, colour)]), cam, "the chain restarts", seeds=1, seed_begin=5)
        r.set_material_data(white, np.array([0.73, 0.73, 0.73], F32))
        alone = frame_copy(r.render(frame, 5, 1))
        assert not np.array_equal(alone["radiance"], chained["radiance"])  # (the chained frame had looked into seed 4's grids)
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_kept_scene_follows_a_device_pointer(built):
    """set_images from a device pointer (an RGBA8 and an RGBA32F image of one mixed scene) and a constant edit, then a transform
    update that moves an instance of the merged mesh: the scene is built again from the kept copy, which must have fetched the
    texels first."""
    import torch

    flags = ["~raycones"]
    moved = translate((0.05, 0.0, -0.05))
    floats, cam = box_scene(False, mirror=False)
    sc = copy.copy(floats)
    sc.images = list(floats.images)
    sc.images[3] = params_bytes(False)  # (image 3 is resident as RGBA8, the others as RGBA32F)
    noise = base_image(1, 7, F32, 90)
    wall = record_address(sc, (0.8, 0.75, 0.7))
    colour = np.array([0.2, 0.9, 0.4], F32)
    r = make_renderer(flags)
    try:
        r.update(sc)
        dev = {3: torch.from_numpy(params_bytes(True)).to("cuda:0"), 2: torch.from_numpy(noise).to("cuda:0")}
        torch.cuda.synchronize()
        info = r.set_images(dev, device_ptr=True)
        assert (info["has_specular_before"], info["has_specular_after"]) == (0, 1)
        r.set_material_data(wall, colour)
        rebuilds = r.stats()["full_rebuilds"]
        sc.set_instance_transform(0, moved)
        r.update_transforms(sc)
        assert r.stats()["full_rebuilds"] == rebuilds + 1
        got = frame_copy(r.render(frame_of(cam), 0, 2))
        want_scene = edited(sc, [(wall, colour)])
        want_scene.images = list(sc.images)
        want_scene.images[3], want_scene.images[2] = params_bytes(True), noise
        same_frame(got, fresh_frame(want_scene, cam, flags), "after the rebuild")
        against_the_oracle(r, got, decoded(want_scene), cam, "after the rebuild")
        assert np.array_equal(r.read_image(3, 0), params_bytes(True)) and np.array_equal(r.read_image(2, 0).view(np.uint32), noise.view(np.uint32))
        assert same_range(r.read_image_range(3), np_range(params_bytes(True)))
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_a_frame_in_flight_completes_with_the_materials_before(built):
    flags = ["~raycones"]
    sc, cam = box_scene(False, mirror=False)
    frame = frame_of(cam)
    metal = record_address(sc, (0.9, 0.7, 0.4))
    colour = np.array([0.1, 0.2, 0.9], F32)
    r = make_renderer(flags)
    try:
        r.update(sc)
        old = frame_copy(r.render(frame, 0, 2))
        ticket = r.render_async(frame, 0, 2)
        r.set_images({3: params_after(False, True)})
        same_frame(frame_copy(r.wait(ticket)), old, "the ticket in flight, images")
        ticket = r.render_async(frame, 0, 2)
        r.set_material_data(metal, colour)
        mirror = fresh_frame(box_scene(False, mirror=True)[0], cam, flags)
        same_frame(frame_copy(r.wait(ticket)), mirror, "the ticket in flight, constants")
        new = frame_copy(r.wait(r.render_async(frame, 0, 2)))
        same_frame(new, fresh_frame(edited(box_scene(False, mirror=True)[0], [(metal, colour)]), cam, flags), "the next frame")
        against_the_oracle(r, new, edited(box_scene(False, mirror=True)[0], [(metal, colour)]), cam, "the next frame")
        assert not np.array_equal(new["radiance"], mirror["radiance"]) and not np.array_equal(mirror["radiance"], old["radiance"])
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_refusals_leave_the_scene_as_it_was(built):
    import torch

    from stratum_amd import _lib

    flags = ["alphatest"]
    sc, cam = foliage_scene(70)
    frame = frame_of(cam)
    leaf = record_address(sc, (0.15, 0.55, 0.1))
    L = _lib.lib()
    r = make_renderer(flags)
    try:
        mask0 = sc.images1[0]
        with pytest.raises(_lib.StratumHipError, match=r"\(-1\).*no scene"):
            r._check(L.sthip_scene_set_images(r._h, None, 0, 32, None), "sthip_scene_set_images")
        with pytest.raises(_lib.StratumHipError, match=r"\(-1\).*no scene"):
            r._check(L.sthip_scene_set_material_data(r._h, 0, wire.ptr(np.zeros(4, np.uint8)), 4, None), "sthip_scene_set_material_data")
        with pytest.raises(_lib.StratumHipError, match=r"\(-1\).*before sthip_scene_upload"):
            r.read_image_range(0)
        r.update(sc)
        before = frame_copy(r.render(frame, 0, 2))
        materials = sc.materials.copy()
        state = {"frame": frame, "before": before}

        def unchanged(what):  # after each refusal the context renders the pre-call frame bit for bit
            same_frame(frame_copy(r.render(state["frame"], 0, 2)), state["before"], "after the refusal: " + what)

        def refused(code, text, entries, struct_size=32):
            arr = (wire.ImageUpdate * max(1, len(entries)))()
            for e, (which, index, pixels, w, h, dev) in zip(arr, entries):
                e.which, e.index, e.pixels, e.width, e.height, e.device_ptr = which, index, pixels, w, h, dev
            with pytest.raises(_lib.StratumHipError, match=r"\(%d\).*%s" % (code, text)):
                r._check(L.sthip_scene_set_images(r._h, arr, len(entries), struct_size, None), "sthip_scene_set_images")
            unchanged(text)

        other = np.ascontiguousarray(255 - mask0)
        p = other.ctypes.data
        refused(-1, "struct_size", [(1, 0, p, 7, 5, 0)], struct_size=24)
        refused(-1, "which", [(2, 0, p, 7, 5, 0)])
        refused(-1, "not in gImage1s", [(1, 2, p, 7, 5, 0)])
        refused(-1, "not in gImages", [(0, 0, p, 7, 5, 0)])  # (the foliage has no image of gImages)
        refused(-1, "pixels is NULL", [(1, 0, None, 7, 5, 0)])
        refused(-1, "extent", [(1, 0, p, 5, 7, 0)])
        refused(-1, "named twice", [(1, 0, p, 7, 5, 0), (1, 1, p, 5, 7, 0), (1, 0, p, 7, 5, 0)])
        dev = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
        refused(-1, "aligned to 4", [(1, 0, dev.data_ptr() + 1, 7, 5, 1)])
        refused(-1, "aligned to 4", [(1, 1, dev.data_ptr() + 2, 5, 7, 1)])

        def refused_data(code, text, offset, data):
            with pytest.raises(_lib.StratumHipError, match=r"\(%d\).*%s" % (code, text)):
                r.set_material_data(offset, data)
            unchanged(text)

        refused_data(-1, "multiples of 4", leaf + 2, np.zeros(4, np.uint8))
        refused_data(-1, "multiples of 4", leaf, np.zeros(6, np.uint8))
        refused_data(-1, "ends past", sc.materials.size - 4, np.zeros(8, np.uint8))
        refused_data(-1, "not in gImages", leaf + 16, np.array([0], np.uint32))
        refused_data(-1, "not in gImage1s", leaf + 60, np.array([2], np.uint32))
        refused_data(-4, "alpha_mask_index", leaf + 60, np.array([0xFFFFFFFF], np.uint32))
        refused_data(-4, "emission", leaf + 12, np.array([3.0], F32))
        with pytest.raises(_lib.StratumHipError, match=r"\(-1\).*data is NULL"):
            r._check(L.sthip_scene_set_material_data(r._h, 0, None, 4, None), "sthip_scene_set_material_data")
        unchanged("data is NULL")
        assert np.array_equal(sc.materials, materials)  # (the scene object follows accepted calls only)
        # a float image at a device pointer that is 4 bytes off, and the environment call's refusal of a shared image
        shared, sky_cam = sky_scene(share=True)
        r.update(shared)
        state["frame"] = frame_of(sky_cam)
        state["before"] = frame_copy(r.render(state["frame"], 0, 2))
        devf = torch.zeros(16 * 32 * 4 + 4, dtype=torch.float32, device="cuda:0")
        refused(-1, "aligned to 16", [(0, 0, devf.data_ptr() + 4, 32, 16, 1)])
        with pytest.raises(_lib.StratumHipError, match=r"\(-4\).*material record"):
            r.set_environment(image=np.ascontiguousarray(shared.images[0] * F32(0.5)))
        unchanged("the environment call's refusal of a shared image")
        with pytest.raises(_lib.StratumHipError, match=r"\(-1\).*extent"):
            r.set_images({0: np.zeros((32, 16, 4), F32)})
        unchanged("a float image of another extent")
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_parity_with_poisoned_allocations(built):
    """One repainted-image case, the binding case and one range case once more in a fresh child process with STHIP_POISON_ALLOC
    (read once per process): every new device buffer starts as 0x7F bytes, the partials and results of the scan among them; a
    fold that read a partial nobody wrote would show."""
    if os.environ.get("STHIP_MATERIAL_POISON_CHILD"):
        return  # (this is the child)
    env = dict(os.environ, STHIP_POISON_ALLOC="0x7F", STHIP_MATERIAL_POISON_CHILD="1")
    select = "repainted_parameter_image and rough_to_mirror or starts_binding or (range_kernel and three_blocks)"
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", select], env=env, cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "failed" not in out.stdout
