"""8-bit resident textures (include/sthip.h: sthip_image_format, sthip_scene_upload_formats, sthip_scene_read_image).

An RGBA8 image of gImages and an R8 mask of gImage1s go up and stay resident as bytes. The contract: a byte b decodes to
float32(b) / float32(255); the mip chain of an RGBA8 image has the shape of the float chain and each channel of a level is the
integer (a + b + c + d + 2) >> 2 over the four clamped source texels, built on the device (csrc/mips.hip); filtering is the
float path's arithmetic on decoded texels. oracle/ knows float images only, so the oracle of the 8-bit path is the FLOAT path:
wherever only level 0 is read (eRayCones off, the alpha test) an 8-bit image must give, bit for bit, what the float image
bytes / 255 gives, and so at every level for a "mip-exact" image, one whose float chain equals its decoded byte chain.
"""
import copy
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stratum_amd import camera, scenes, wire  # noqa: E402
from stratum_amd.scene import translate  # noqa: E402

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------------
# the contract in numpy (the reference of the read-back test)
# ---------------------------------------------------------------------------------------------------------------------------
def decode(b):
    """A byte is the correctly rounded binary32 quotient b / 255 (numpy divides float32 by float32 in float32: IEEE)."""
    return np.asarray(b, np.uint8).astype(F32) / F32(255)


def _taps(level):
    h, w = level.shape[:2]
    nh, nw = max(1, h // 2), max(1, w // 2)
    y, x = np.arange(nh), np.arange(nw)
    y0, y1, x0, x1 = np.minimum(2 * y, h - 1), np.minimum(2 * y + 1, h - 1), np.minimum(2 * x, w - 1), np.minimum(2 * x + 1, w - 1)
    return level[y0][:, x0], level[y0][:, x1], level[y1][:, x0], level[y1][:, x1]


def byte_chain(image):
    """The levels of an RGBA8 (H, W, 4) image: max(1, dim // 2), clamped taps, (a + b + c + d + 2) >> 2 in integers."""
    levels = [np.ascontiguousarray(image, np.uint8)]
    while levels[-1].shape[:2] != (1, 1) and len(levels) < wire.MAX_MIPS:
        a, b, c, d = (t.astype(np.uint32) for t in _taps(levels[-1]))
        levels.append(((a + b + c + d + 2) >> 2).astype(np.uint8))
    return levels


def float_chain(image):
    """The levels of a float image as sthip_scene_upload builds them: ((a + b) + (c + d)) * 0.25f over the same taps."""
    levels = [np.ascontiguousarray(image, F32)]
    while levels[-1].shape[:2] != (1, 1) and len(levels) < wire.MAX_MIPS:
        a, b, c, d = _taps(levels[-1])
        levels.append(((a + b) + (c + d)) * F32(0.25))
    return levels


def mip_exact_image(n, seed, channels=4):
    """A random n x n byte image (n a power of two) whose float chain equals its decoded byte chain at every level. Top-down:
    from a 1 x 1 value, every texel t is split into four bytes with a + b + c + d = 4 t (so the integer mean is t) that also
    satisfy ((da + db) + (dc + dd)) * 0.25f == decode(t) in float32. Most quadruples with an integral mean qualify; a draw
    that does not is drawn again."""
    rng = np.random.RandomState(seed)
    level = rng.randint(96, 160, size=(1, 1, channels)).astype(np.int64)
    quarter = F32(0.25)
    while level.shape[0] < n:
        h, w = level.shape[:2]
        nxt = np.zeros((2 * h, 2 * w, channels), np.int64)
        for y in range(h):
            for x in range(w):
                for k in range(channels):
                    t = int(level[y, x, k])
                    spread = min(48, t, 255 - t)  # (the four stay inside 0 .. 255 more often than not)
                    for _ in range(10000):
                        a, b, c = (int(v) for v in t + rng.randint(-spread, spread + 1, size=3))
                        d = 4 * t - a - b - c
                        if min(a, b, c, d) < 0 or max(a, b, c, d) > 255:
                            continue
                        da, db, dc, dd = (decode(v) for v in (a, b, c, d))
                        if ((da + db) + (dc + dd)) * quarter == decode(t):
                            break
                    else:
                        raise AssertionError("no mip-exact split of %d" % t)
                    nxt[2 * y, 2 * x, k], nxt[2 * y, 2 * x + 1, k], nxt[2 * y + 1, 2 * x, k], nxt[2 * y + 1, 2 * x + 1, k] = a, b, c, d
        level = nxt
    return level.astype(np.uint8)


def is_mip_exact(image):
    return all(np.array_equal(f.view(np.uint32), decode(b).view(np.uint32)) for f, b in zip(float_chain(decode(image)), byte_chain(image)))


def random_bytes(h, w, seed, channels=4):
    """Random bytes with the ends of the range over-represented (0 and 255: the texels the specular bound turns on); an image
    of 256 texels holds every byte value in every channel, so the decode is checked for all of them."""
    rng = np.random.RandomState(seed)
    if h * w == 256:
        return np.ascontiguousarray(np.stack([rng.permutation(256) for _ in range(channels)], -1).reshape(h, w, channels).astype(np.uint8))
    img = rng.randint(0, 256, size=(h, w, channels))
    pick = rng.rand(h, w, channels)
    img[pick < 0.1] = 0
    img[pick > 0.9] = 255
    return np.ascontiguousarray(img.astype(np.uint8))


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sthip.h")).read(), flags=re.S)


def test_header_loader_and_wire_agree_on_the_new_symbols(built):
    from stratum_amd import _lib

    text = _header()
    assert re.search(r"int\s+sthip_scene_upload_formats\s*\(\s*sthip_ctx\s*\*\s*\w+\s*,\s*const\s+sthip_scene_desc\s*\*\s*\w+\s*,\s*const\s+uint8_t\s*\*\s*image_formats\s*,\s*const\s+uint8_t\s*\*\s*image1_formats\s*\)", text)
    assert re.search(r"int\s+sthip_scene_read_image\s*\(\s*sthip_ctx\s*\*\s*\w+\s*,\s*uint32_t\s+image_index\s*,\s*uint32_t\s+level\s*,\s*void\s*\*\s*out\s*,\s*uint64_t\s+out_bytes\s*\)", text)
    values = {name: int(v) for name, v in re.findall(r"(STHIP_IMAGE_FORMAT_\w+)\s*=\s*(\d+)", text)}
    assert values == {"STHIP_IMAGE_FORMAT_RGBA32F": 0, "STHIP_IMAGE_FORMAT_RGBA8_UNORM": 1, "STHIP_IMAGE_FORMAT_R32F": 0, "STHIP_IMAGE_FORMAT_R8_UNORM": 1}
    for name, v in values.items():
        assert getattr(wire, name[len("STHIP_") :]) == v
    shading = open(os.path.join(ROOT, "stratum_amd", "csrc", "bvh.h")).read()  # (DeviceImage and its level count live there)
    assert int(re.search(r"#define\s+STHIP_MAX_MIPS\s+(\d+)", shading).group(1)) == wire.MAX_MIPS
    L = _lib.lib()
    for name in ("sthip_scene_upload_formats", "sthip_scene_read_image"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.sthip_abi_version() == 11 and "#define STHIP_ABI_VERSION 11" in text


def test_numpy_statement_of_the_contract():
    d = decode(np.arange(256))
    assert d.dtype == F32 and d[0] == 0 and d[255] == 1 and np.all(np.diff(d) > 0)
    exact = np.arange(256, dtype=np.float64) / 255.0  # the real quotient to 53 bits: its float32 rounding is the decode
    assert np.array_equal(d, exact.astype(F32))
    # 5 x 3 (W x H): levels 2 x 1 and 1 x 1, the odd column and the odd row never read past the clamp
    img = random_bytes(3, 5, 1)
    chain = byte_chain(img)
    assert [lv.shape for lv in chain] == [(3, 5, 4), (1, 2, 4), (1, 1, 4)]
    i = img.astype(np.int64)
    assert np.array_equal(chain[1][0, 0], (i[0, 0] + i[0, 1] + i[1, 0] + i[1, 1] + 2) >> 2)
    assert np.array_equal(chain[1][0, 1], (i[0, 2] + i[0, 3] + i[1, 2] + i[1, 3] + 2) >> 2)
    c1 = chain[1].astype(np.int64)
    assert np.array_equal(chain[2][0, 0], (2 * c1[0, 0] + 2 * c1[0, 1] + 2) >> 2)  # (height 1: both rows clamp to row 0)
    # 1 x 7 (W x H): width stays 1, the taps of a column are the same texel twice
    img = random_bytes(7, 1, 2)
    chain = byte_chain(img)
    assert [lv.shape for lv in chain] == [(7, 1, 4), (3, 1, 4), (1, 1, 4)]
    i = img.astype(np.int64)
    assert np.array_equal(chain[1][2, 0], (2 * i[4, 0] + 2 * i[5, 0] + 2) >> 2)
    # 1 x 1: one level
    img = random_bytes(1, 1, 3)
    assert len(byte_chain(img)) == 1 and np.array_equal(byte_chain(img)[0], img)
    assert [lv.shape for lv in float_chain(decode(random_bytes(3, 5, 1)))] == [(3, 5, 4), (1, 2, 4), (1, 1, 4)]
    assert len(byte_chain(np.zeros((16, 16, 4), np.uint8))) == 5


@functools.lru_cache(maxsize=None)
def exact_image(seed):
    return mip_exact_image(16, seed)


def test_mip_exact_images_have_equal_chains():
    img = exact_image(11)
    assert img.shape == (16, 16, 4) and img.dtype == np.uint8
    assert len(np.unique(img)) >= 64  # (not a flat image: the levels above 0 differ from level 0)
    assert is_mip_exact(img)
    assert not np.array_equal(byte_chain(img)[1], img[::2, ::2])
    # ... and a random image is not: the property is worth generating for
    assert not is_mip_exact(random_bytes(16, 16, 4))
    assert all(len(np.unique(random_bytes(16, 16, 4)[..., k])) == 256 for k in range(4))


def test_scene_formats_follow_the_dtype():
    sc, _ = small_textured(False, "bytes")
    f, f1 = sc.formats()
    assert f.dtype == np.uint8 and f.tolist() == [1] * len(sc.images) and f1.size == 0
    sc, _ = small_textured(False, "float")
    assert sc.formats()[0].tolist() == [0] * len(sc.images)
    from stratum_amd.scene import SceneBuilder

    b = SceneBuilder()
    assert b._images == [] and b.add_image(np.zeros((2, 2, 4), np.uint8)) == 0 and b._images[0].dtype == np.uint8
    assert b.add_image(np.zeros((2, 2, 4))) == 1 and b._images[1].dtype == F32
    assert b.add_image1(np.zeros((2, 2), np.uint8)) == 0 and b._images1[0].dtype == np.uint8


# ---------------------------------------------------------------------------------------------------------------------------
# scenes: the textured box and the foliage with small images
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _textured(mirror_map):
    return scenes.textured_box(mirror_map=mirror_map)


SIZES = [(16, 16), (3, 5), (7, 1), (16, 16), (1, 1)]  # (H, W) of the five images of textured_box, in gImages order


def small_textured(mirror_map, kind, order=None):
    """textured_box with every image replaced. kind "bytes": random bytes, uploaded as RGBA8; "float": the same texels as
    float32 (bytes / 255); "exact" / "exact-float": 16 x 16 mip-exact images; order: per image 1 = bytes, 0 = float."""
    base, cam = _textured(mirror_map)
    sc = copy.copy(base)
    if kind.startswith("exact"):
        images = [exact_image(20 + i) for i in range(len(base.images))]
    else:
        images = [random_bytes(h, w, 40 + i) for i, (h, w) in enumerate(SIZES[: len(base.images)])]
    assert len(images) == len(base.images) == 5
    if mirror_map:  # the roughness map (image 3): G = 0 texels make the metal ball specular there, by the texels alone
        assert (images[3][..., 1] == 0).any() or kind.startswith("exact")
    as_bytes = order if order is not None else [0 if kind.endswith("float") else 1] * len(images)
    sc.images = [img if b else decode(img) for img, b in zip(images, as_bytes)]
    return sc, cam


def mask_bytes(h, w, seed):
    """Coverage bytes around the 0.75 threshold of the alpha test: 191 / 255 < 0.75 <= 192 / 255, and their neighbours."""
    rng = np.random.RandomState(seed)
    return np.ascontiguousarray(rng.choice(np.array([0, 64, 189, 190, 191, 192, 193, 194, 255], np.uint8), size=(h, w)))


@functools.lru_cache(maxsize=None)
def _foliage():
    return scenes.foliage()


def small_foliage(as_bytes, size):
    base, cam = _foliage()
    sc = copy.copy(base)
    assert len(base.images1) == 2
    masks = [mask_bytes(size[0], size[1], 70), mask_bytes(size[1], size[0], 71)]
    sc.images1 = [m if as_bytes else decode(m) for m in masks]
    return sc, cam


def make_renderer(flags=(), options=None, args=None):
    from stratum_amd.bdpt import BDPT

    r = BDPT(device=0, args=dict(args or {}, bdptFlag=list(flags)))
    for k, v in (options or {}).items():
        r.set_option(k, v)
    return r


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(-1)


def same_frame(a, b, what=""):
    for k in ("radiance", "albedo", "visibility", "depth", "prev_uv", "ray_count"):
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k)


def frame_copy(out):
    return {k: np.array(v, copy=True) for k, v in out.items() if isinstance(v, np.ndarray)}


def render(sc, cam, flags=(), options=None, size=(64, 48), seeds=2, args=None):
    frame = camera.Frame(size[0], size[1], cam["fovy"], cam["eye"], cam["target"])
    r = make_renderer(flags, options, args)
    try:
        r.update(sc)
        return frame_copy(r.render(frame, 0, seeds))
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mip_chain_read_back(built):
    """Every level of 16 x 16, 5 x 3, 1 x 7 and 1 x 1 RGBA8 images as sthip_scene_read_image returns it equals the numpy statement
    (level 0: the uploaded bytes); a float image in the same scene reads back the float chain."""
    order = [1, 1, 1, 0, 1]
    sc, _ = small_textured(False, "bytes", order=order)
    r = make_renderer()
    try:
        r.update(sc)
        for index, img in enumerate(sc.images):
            if img.dtype == np.uint8:
                chain = byte_chain(img)
                assert np.array_equal(r.read_image(index, 0), img)
            else:
                chain = float_chain(img)
            for level, want in enumerate(chain):
                got = r.read_image(index, level)
                assert got.dtype == want.dtype and got.shape == want.shape, (index, level)
                assert np.array_equal(bits(got), bits(want)), (index, level)
        assert [len(byte_chain(i)) for i in sc.images if i.dtype == np.uint8] == [5, 3, 3, 1]
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("normal_maps", [True, False])
@pytest.mark.parametrize("mirror_map", [False, True])
def test_level_0_parity_with_the_float_upload(built, mirror_map, normal_maps):
    """Without eRayCones every lookup reads level 0 alone: random bytes uploaded as RGBA8 give the frame of the float upload of
    bytes / 255 bit for bit — base colour, parameter, bump and light images; the mirror map goes through the host's bound."""
    flags = ["~raycones"] + ([] if normal_maps else ["~normalmaps"])
    a = render(*small_textured(mirror_map, "bytes"), flags=flags)
    b = render(*small_textured(mirror_map, "float"), flags=flags)
    same_frame(a, b, "8-bit against float")
    assert a["radiance"][..., :3].any() and a["ray_count"][0] > 0
    if mirror_map and normal_maps:  # ... and the float frame is the oracle's
        from oracle import oracle_py

        sc, cam = small_textured(mirror_map, "float")
        frame = camera.Frame(64, 48, cam["fovy"], cam["eye"], cam["target"])
        r = make_renderer(flags)
        try:
            r.update(sc)  # (push_constants takes the light count from the bound scene)
            ref = oracle_py.OracleScene(sc).render(frame, r.push_constants(frame), r.mSamplingFlags, 0, 2)
        finally:
            r.close()
        differing = int((a["radiance"].view(np.uint32) != ref["radiance"].view(np.uint32)).any(axis=-1).sum())
        print("8-bit frame against the oracle of the float scene: %d of %d radiance pixels differ" % (differing, 64 * 48))
        for k in ("radiance", "albedo"):
            assert np.array_equal(bits(a[k]), bits(ref[k])), k
        assert np.array_equal(a["visibility"]["instance_primitive_index"], ref["visibility"]["instance_primitive_index"])
        assert np.array_equal(a["ray_count"], ref["ray_count"])


@pytest.mark.gpu
def test_the_images_matter(built):
    """The parity tests discriminate: other bytes give another frame."""
    sc, cam = small_textured(False, "bytes")
    a = render(sc, cam, flags=["~raycones"])
    sc2 = copy.copy(sc)
    sc2.images = [np.ascontiguousarray(255 - img) for img in sc.images]
    b = render(sc2, cam, flags=["~raycones"])
    assert not np.array_equal(bits(a["radiance"]), bits(b["radiance"]))


@pytest.mark.gpu
def test_ray_cones_on_mip_exact_images(built):
    """eRayCones on: the trilinear path reads levels above 0. For images whose float chain equals their decoded byte chain the
    8-bit upload gives the float upload's frame bit for bit."""
    a = render(*small_textured(False, "exact"), flags=["raycones"])
    b = render(*small_textured(False, "exact-float"), flags=["raycones"])
    same_frame(a, b, "ray cones")
    c = render(*small_textured(False, "exact"), flags=["~raycones"])
    assert not np.array_equal(bits(a["radiance"]), bits(c["radiance"]))  # (levels above 0 were read)


@pytest.mark.gpu
@pytest.mark.parametrize("order", [[1, 0, 1, 0, 1], [0, 1, 0, 1, 0]])
def test_mixed_formats_in_one_scene(built, order):
    """Float and 8-bit images side by side, in both index orders: the offsets of one format do not disturb the other."""
    a = render(*small_textured(True, "bytes", order=order), flags=["~raycones"])
    b = render(*small_textured(True, "float"), flags=["~raycones"])
    same_frame(a, b, "mixed %s" % order)


def _mask_rays(n=4096, seed=5):
    rng = np.random.RandomState(seed)
    rays = np.zeros(n, wire.Ray)
    origin = np.stack([rng.uniform(-2, 2, n), np.full(n, 3.5), rng.uniform(-2, 1.5, n)], 1)
    target = np.stack([rng.uniform(-2, 2, n), np.zeros(n), rng.uniform(-2, 1.5, n)], 1)
    d = target - origin
    rays["origin"], rays["direction"] = origin, d / np.linalg.norm(d, axis=1, keepdims=True)
    rays["tmin"], rays["tmax"] = 0, 1e30
    return rays


@pytest.mark.gpu
@pytest.mark.parametrize("flip_uvs", [False, True])
@pytest.mark.parametrize("builder", [0, 1])
@pytest.mark.parametrize("size", [(5, 7), (16, 16)], ids=["7x5", "16x16"])
def test_alpha_masks_as_bytes(built, size, builder, flip_uvs):
    """R8 masks with bytes around the 0.75 threshold, eAlphaTest: closest-hit and shadow rays through sthip_render and
    sthip_trace_rays (any_hit 0 and 1) give what the float masks bytes / 255 give; without the test the frame differs."""
    flags = ["alphatest"] + (["fliptriangleuvs"] if flip_uvs else [])
    options = {"bvh_builder": builder}
    frames, hits = [], []
    for as_bytes in (True, False):
        sc, cam = small_foliage(as_bytes, size)
        frame = camera.Frame(64, 48, cam["fovy"], cam["eye"], cam["target"])
        r = make_renderer(flags, options)
        try:
            r.update(sc)
            frames.append(frame_copy(r.render(frame, 0, 2)))
            hits.append([r.trace(_mask_rays(), any_hit=a, alpha_test=True, flip_uvs=flip_uvs).copy() for a in (False, True)])
            if as_bytes:
                solid = r.trace(_mask_rays(), any_hit=False, alpha_test=False, flip_uvs=flip_uvs).copy()
        finally:
            r.close()
    same_frame(frames[0], frames[1], "masks")
    for a, b in zip(hits[0], hits[1]):
        assert np.array_equal(bits(a), bits(b))
    # the comparison discriminates: the mask cuts rays the solid cards stop
    assert not np.array_equal(hits[0][0]["instance_primitive_index"], solid["instance_primitive_index"])


@pytest.mark.gpu
def test_mask_threshold_bytes(built):
    """191 / 255 < 0.75 <= 192 / 255: a mask of 191s is all holes, a mask of 192s is solid."""
    rays = _mask_rays(1024)
    got = []
    for value in (191, 192):
        base, _ = _foliage()
        sc = copy.copy(base)
        sc.images1 = [np.full((4, 4), value, np.uint8), np.full((4, 4), value, np.uint8)]
        r = make_renderer()
        try:
            r.update(sc)
            got.append(r.trace(rays, alpha_test=True).copy())
            solid = r.trace(rays, alpha_test=False).copy()
        finally:
            r.close()
    assert np.array_equal(bits(got[1]), bits(solid)) and not np.array_equal(bits(got[0]), bits(solid))


@pytest.mark.gpu
def test_rebuilds_from_the_kept_scene_keep_the_formats(built):
    """An instance of the merged mesh moves: sthip_scene_update_transforms builds the scene again from the kept copy, which
    holds the 8-bit images as bytes with their formats; the frame is the one of a fresh upload of the moved scene. Once more
    with sthip_scene_update_vertices on a layout the refit does not serve."""
    sc, cam = small_textured(True, "bytes", order=[1, 0, 1, 1, 1])
    sc = copy.deepcopy(sc)
    frame = camera.Frame(64, 48, cam["fovy"], cam["eye"], cam["target"])
    flags = ["~raycones"]
    r = make_renderer(flags)
    try:
        r.update(sc)
        before = frame_copy(r.render(frame, 0, 1))
        sc.set_instance_transform(0, translate((0.0, 0.15, 0.0)))  # the floor: identity at upload, part of the merged mesh
        r.update_transforms(sc)
        assert r.stats()["full_rebuilds"] == 1
        moved = frame_copy(r.render(frame, 0, 1))
        assert np.array_equal(r.read_image(0, 1), byte_chain(sc.images[0])[1])
    finally:
        r.close()
    fresh = render(sc, cam, flags=flags, seeds=1)
    for k in ("radiance", "albedo", "visibility", "depth", "ray_count"):
        assert np.array_equal(bits(moved[k]), bits(fresh[k])), k
    assert not np.array_equal(bits(moved["radiance"]), bits(before["radiance"]))

    sc, cam = small_textured(True, "bytes", order=[1, 0, 1, 1, 1])
    sc = copy.deepcopy(sc)
    r = make_renderer(flags, {"treetop": 1})
    try:
        r.update(sc)
        v = sc.vertices[40:200].copy()
        v["position"] = v["position"] * F32(0.9)
        sc.set_vertices(40, v)
        assert r.update_vertices(sc)["rebuilt"] == 1
        deformed = frame_copy(r.render(frame, 0, 1))
    finally:
        r.close()
    fresh = render(sc, cam, flags=flags, options={"treetop": 1}, seeds=1)
    for k in ("radiance", "albedo", "visibility", "depth", "ray_count"):
        assert np.array_equal(bits(deformed[k]), bits(fresh[k])), k


@pytest.mark.gpu
def test_refusals(built):
    from stratum_amd import _lib
    from stratum_amd.bdpt import StratumHipError

    L = _lib.lib()
    # an 8-bit environment map: refused at render, with a message
    sc, cam = scenes.environment_scene(image=True, emitter=True)
    sc = copy.copy(sc)
    env = len(sc.images) - 1
    sc.images = list(sc.images)
    sc.images[env] = np.ascontiguousarray((np.clip(sc.images[env], 0, 1) * 255).astype(np.uint8))
    frame = camera.Frame(32, 24, cam["fovy"], cam["eye"], cam["target"])
    r = make_renderer()
    try:
        r.update(sc)
        with pytest.raises(StratumHipError) as e:
            r.render(frame, 0, 1)
        assert "(-4)" in str(e.value) and "environment" in str(e.value) and "8-bit" in str(e.value)
    finally:
        r.close()
    # format 2 is no format; sthip_scene_read_image out of range
    sc, _ = small_textured(False, "bytes")
    r = make_renderer()
    try:
        d = sc.desc()
        bad = np.array([1, 1, 2, 1, 1], np.uint8)
        assert L.sthip_scene_upload_formats(r._h, C.byref(d), wire.ptr(bad), None) == -1
        assert b"image_formats[2]" in L.sthip_last_error(r._h)
        out = np.zeros((16, 16, 4), np.uint8)
        assert L.sthip_scene_read_image(r._h, 0, 0, wire.ptr(out), out.nbytes) == -1  # no scene
        r.update(sc)
        assert L.sthip_scene_read_image(r._h, 0, 0, wire.ptr(out), out.nbytes) == 0
        assert L.sthip_scene_read_image(r._h, 5, 0, wire.ptr(out), out.nbytes) == -1
        assert L.sthip_scene_read_image(r._h, 0, 5, wire.ptr(out), 4) == -1
        assert L.sthip_scene_read_image(r._h, 0, 0, wire.ptr(out), out.nbytes - 4) == -1
        assert L.sthip_scene_read_image(r._h, 0, 0, None, out.nbytes) == -1
        assert L.sthip_last_error(r._h)
        # a mask format that is none
        fsc, _ = small_foliage(True, (5, 7))
        d = fsc.desc()
        assert L.sthip_scene_upload_formats(r._h, C.byref(d), None, wire.ptr(np.array([1, 3], np.uint8))) == -1
        assert b"image1_formats[1]" in L.sthip_last_error(r._h)
        # NULL arrays: sthip_scene_upload
        d = sc.desc()
        fl = copy.copy(sc)
        fl.images = [decode(i) for i in sc.images]
        d = fl.desc()
        assert L.sthip_scene_upload_formats(r._h, C.byref(d), None, None) == 0
        got = np.zeros((16, 16, 4), F32)
        assert L.sthip_scene_read_image(r._h, 0, 0, wire.ptr(got), got.nbytes) == 0 and np.array_equal(got, fl.images[0])
    finally:
        r.close()


@pytest.mark.gpu
def test_8_bit_images_with_poisoned_allocations(built):
    """The read-back and one parity case once more in a fresh child process with STHIP_POISON_ALLOC (read once per process):
    every new device buffer starts as 0x7F bytes, so a level or a padding byte that is read before it is written shows."""
    if os.environ.get("STHIP_IMAGE_FORMATS_POISON_CHILD"):
        return  # (this is the child)
    env = dict(os.environ, STHIP_POISON_ALLOC="0x7F", STHIP_IMAGE_FORMATS_POISON_CHILD="1")
    out = subprocess.run(
        [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "read_back or ray_cones or (alpha_masks and 7x5-0-False)"],
        env=env, cwd=ROOT, capture_output=True, text=True, timeout=600,
    )
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "failed" not in out.stdout


# ---------------------------------------------------------------------------------------------------------------------------
# the C++ host (stratum_amd/host/stratum_hip.hpp: Image::bytes, Image1::bytes, SceneData::upload)
# ---------------------------------------------------------------------------------------------------------------------------
IMAGE_FORMATS_HOST = os.path.join(ROOT, "tests", "cpp", "image_formats_host")


@pytest.fixture(scope="module")
def image_formats_host(built):
    src = os.path.join(ROOT, "tests", "cpp", "image_formats_host.cpp")
    deps = [src, os.path.join(ROOT, "tests", "cpp", "scene_reader.hpp"), os.path.join(ROOT, "stratum_amd", "host", "stratum_hip.hpp"), os.path.join(ROOT, "include", "sthip.h")]
    if not os.path.exists(IMAGE_FORMATS_HOST) or os.path.getmtime(IMAGE_FORMATS_HOST) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(
            ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-o", IMAGE_FORMATS_HOST, src, "-L" + os.path.join(ROOT, "stratum_amd"), "-lstratum_hip", "-Wl,-rpath," + os.path.join(ROOT, "stratum_amd")]
        )
    return IMAGE_FORMATS_HOST


def card_scene(as_bytes):
    """A textured floor with a normal map, an alpha-masked card over it and a textured light, built through SceneBuilder (what
    dump_description writes for the C++ host): every image either as bytes or as the floats bytes / 255."""
    from stratum_amd.scene import SceneBuilder

    form = (lambda b: b) if as_bytes else decode
    b = SceneBuilder("cards")
    colour = b.add_image(form(random_bytes(16, 16, 90)))
    bump = b.add_image(form(random_bytes(5, 3, 91)))
    glow = b.add_image(form(random_bytes(1, 7, 92)))
    floor = b.add_material((1.0, 1.0, 1.0), roughness=0.4)
    b.set_material_images(floor, base_color_image=colour, bump_image=bump, bump_strength=1.5)
    leaf = b.add_material((0.2, 0.6, 0.1), roughness=0.6)
    b.set_material_alpha_mask(leaf, b.add_image1(form(mask_bytes(5, 7, 93))))
    light = b.add_emitter((17.0, 12.0, 4.0))
    b.set_material_images(light, base_color_image=glow)

    def quad(p0, p1, p2, p3, n, mat, transform=None):
        pos, nrm, uv, tri = scenes._quad(p0, p1, p2, p3, n)
        b.add_instance(b.add_mesh(pos, nrm, uv * 2.0, tri), mat, transform)

    quad((-1, -1, 1), (1, -1, 1), (1, -1, -1), (-1, -1, -1), (0, 1, 0), floor)
    quad((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (0, 0, 1), floor)
    quad((-0.5, 0, 0.5), (0.5, 0, 0.5), (0.5, 0, -0.5), (-0.5, 0, -0.5), (0, 1, 0), leaf, translate((0.0, -0.3, 0.0)))
    quad((-0.3, 0.9, -0.3), (0.3, 0.9, -0.3), (0.3, 0.9, 0.3), (-0.3, 0.9, 0.3), (0, -1, 0), light)
    return b.build(), {"eye": (0.0, 0.2, 3.5), "target": (0.0, -0.2, 0.0), "fovy": np.radians(40.0)}


def test_cpp_host_packs_8_bit_images_as_bytes(image_formats_host, tmp_path):
    """No GPU: without arguments the program prints its usage; Scene::update hands every 8-bit image over as its bytes with
    format 1 (the library has sthip_scene_upload_formats, so nothing is converted to floats on the host)."""
    from stratum_amd.scene import dump_description

    out = subprocess.run([image_formats_host], capture_output=True, text=True)
    assert out.returncode == 2 and "usage: image_formats_host" in out.stderr
    sc, cam = card_scene(False)
    desc = str(tmp_path / "scene.bin")
    dump_description(desc, sc, camera.Frame(64, 48, cam["fovy"], cam["eye"], cam["target"]))
    out = subprocess.run([image_formats_host, "pack", desc], capture_output=True, text=True)
    assert out.returncode == 0 and "PACKED converted=4 images=3 masks=1 as_bytes=4 host_floats=0" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_cpp_host_renders_the_frame_of_the_python_host(image_formats_host, tmp_path):
    """The C++ host with every image as bytes gives, byte for byte, the frame the Python host gives for the uint8 scene (and so
    the 8-bit images went up as such on both sides: the default flags have eRayCones on, where the integer chain is read)."""
    from stratum_amd.scene import dump_description

    W, H, seeds = 64, 48, 2
    sc, cam = card_scene(False)
    fr = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
    desc, outp = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    dump_description(desc, sc, fr)
    out = subprocess.run([image_formats_host, "render", desc, outp, str(seeds)], capture_output=True, text=True)
    assert out.returncode == 0 and "RENDERED converted=4" in out.stdout, out.stdout + out.stderr
    raw = np.fromfile(outp, dtype=np.uint8)
    rad = raw[: W * H * 16].view(F32).reshape(H, W, 4)
    rays = raw[W * H * 16 : W * H * 16 + 16].view(np.uint64)
    sc8, _ = card_scene(True)
    assert sc8.formats()[0].tolist() == [1, 1, 1] and sc8.formats()[1].tolist() == [1]
    assert sc8.materials.tobytes() == sc.materials.tobytes()
    want = render(sc8, cam, size=(W, H), seeds=seeds)
    assert np.array_equal(bits(rad), bits(want["radiance"])) and np.array_equal(rays, want["ray_count"])
    assert rad[..., :3].any()
