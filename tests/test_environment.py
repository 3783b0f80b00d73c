"""sthip_scene_set_environment / sthip_scene_read_distributions (include/sthip.h: "the environment of a resident scene"): the
environment's texels and value replaced in a resident scene, its mip chain and dist2d tables built on the device.

The reference of every comparison is the host: scene.py build_distributions for the tables, a numpy statement of the mip
rule for the chain. Both are pinned here, bit for bit, by tests/cpp/environment_ref.cpp (a scalar C++ restatement written from
the header's text) before anything goes to the GPU. A NaN stands against a NaN; everything else is compared as bytes."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from stratum_amd import camera, scenes, wire  # noqa: E402
from stratum_amd.scene import SceneBuilder, build_distributions, translate  # noqa: E402

F32 = np.float32
OUTPUTS = ("radiance", "albedo", "visibility", "depth", "prev_uv", "ray_count")


# ---------------------------------------------------------------------------------------------------------------------------
# images
# ---------------------------------------------------------------------------------------------------------------------------
EXTENTS = [(1, 1), (2, 1), (3, 5), (17, 33), (65, 129), (130, 257)]  # (H, W): tails of a 64-wide and a 64-row tile; two row tiles


def hdr(h, w, seed):
    """Log-normal HDR values around 1e-2 with one texel of 1e5 (a sun)."""
    rng = np.random.RandomState(seed)
    img = np.ones((h, w, 4), F32)
    img[..., :3] = (1e-2 * np.exp(rng.normal(0.0, 1.0, size=(h, w, 3)))).astype(F32)
    img[h // 3, (2 * w) // 3, :3] = F32(1e5)
    return img


def planted(h, w, seed):
    """hdr with, as far as the height allows: a black row between lit rows (row fallback), a row whose sum is negative, a row
    with a single lit texel, a row of binary32 subnormals, and two more black rows."""
    img = hdr(h, w, seed)
    if h >= 2:
        img[1, :, :3] = 0
    if h >= 5:
        img[3, :, :3] = F32(-0.25)
        img[3, 0, :3] = F32(0.5)  # (lit first: the running sum changes sign on the way)
    if h >= 7:
        img[5, :, :3] = 0
        img[5, w // 2, :3] = F32(3.0)
    if h >= 9:
        img[7, :, :3] = np.array([1e-41, 3e-42, 7e-43], F32)
    if h >= 17:
        img[9:11, :, :3] = 0
    return img


def with_texel(img, value):
    out = img.copy()
    out[out.shape[0] // 2, out.shape[1] // 3, 1] = F32(value)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (H, W, 4) float32 image."""
    out = {}
    for k, (h, w) in enumerate(EXTENTS):
        out["planted_%dx%d" % (h, w)] = planted(h, w, 100 + k)
    for h, w in ((3, 5), (65, 129)):
        img = np.zeros((h, w, 4), F32)
        img[..., 3] = 1
        out["black_%dx%d" % (h, w)] = img  # the marginal fallback
    out["nan_17x33"] = with_texel(planted(17, 33, 7), np.nan)
    out["nan_130x257"] = with_texel(hdr(130, 257, 8), np.nan)
    out["inf_17x33"] = with_texel(hdr(17, 33, 9), np.inf)
    out["inf_65x129"] = with_texel(planted(65, 129, 10), np.inf)
    for v in out.values():
        v.setflags(write=False)
    return out


CASE_NAMES = sorted(cases())


def np_mips(img):
    """The levels above 0 of an RGBA32F image by the rule of include/sthip.h, in numpy float32."""
    levels, cur = [], np.asarray(img, F32)
    while cur.shape[0] > 1 or cur.shape[1] > 1:
        h, w = cur.shape[:2]
        nh, nw = max(1, h // 2), max(1, w // 2)
        y0, y1 = np.minimum(2 * np.arange(nh), h - 1), np.minimum(2 * np.arange(nh) + 1, h - 1)
        x0, x1 = np.minimum(2 * np.arange(nw), w - 1), np.minimum(2 * np.arange(nw) + 1, w - 1)
        with np.errstate(invalid="ignore", over="ignore"):
            a, b, c, e = cur[y0][:, x0], cur[y0][:, x1], cur[y1][:, x0], cur[y1][:, x1]
            cur = (((a + b) + (c + e)) * F32(0.25)).astype(F32)
        levels.append(cur)
    return levels


def same(a, b):
    """Bit for bit, a NaN standing against a NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


@functools.lru_cache(maxsize=None)
def host_tables(name):
    with np.errstate(all="ignore"):
        t = np.concatenate(build_distributions(cases()[name])).astype(F32)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def host_mips(name):
    return np_mips(cases()[name])


# ---------------------------------------------------------------------------------------------------------------------------
# the C++ restatement pins the reference
# ---------------------------------------------------------------------------------------------------------------------------
REF_SRC = os.path.join(ROOT, "tests", "cpp", "environment_ref.cpp")
CHECK_SRC = os.path.join(ROOT, "tests", "cpp", "environment_check.cpp")
CXX = os.environ.get("CXX", "g++")


def run_ref(exe, tmp, mode, img):
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array(img.shape[:2], np.uint32).tobytes())
        f.write(np.ascontiguousarray(img, F32).tobytes())
    subprocess.check_call([exe, mode, fin, fout])
    return np.fromfile(fout, F32)


@pytest.fixture(scope="module")
def pinned(tmp_path_factory):
    """The host references of every case, after the C++ restatement has agreed with them bit for bit."""
    tmp = str(tmp_path_factory.mktemp("environment_ref"))
    exe = os.path.join(tmp, "environment_ref")
    subprocess.check_call([CXX, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-o", exe, REF_SRC])
    for name in CASE_NAMES:
        img = cases()[name]
        assert same(run_ref(exe, tmp, "tables", img), host_tables(name)), name
        levels = host_mips(name)
        want = np.concatenate([lv.reshape(-1) for lv in levels]) if levels else np.zeros(0, F32)
        assert same(run_ref(exe, tmp, "mips", img), want), name
    return {name: (host_tables(name), host_mips(name)) for name in CASE_NAMES}


# ---------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_library_exports_and_header_declares_both_symbols(built):
    from stratum_amd import _lib

    L = _lib.lib()
    hdr_text = open(os.path.join(ROOT, "include", "sthip.h")).read()
    for name in ("sthip_scene_set_environment", "sthip_scene_read_distributions"):
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
        assert re.search(r"^int %s\(sthip_ctx\*" % name, hdr_text, re.M), name
    assert L.sthip_abi_version() == 11 and "#define STHIP_ABI_VERSION 11" in hdr_text
    for phrase in ("typedef struct sthip_environment_desc", "((a + b) + (c + e)) * 0.25f", "(r*0.2126f + g*0.7152f) + b*0.0722f", "row[x+1] = (float)((double)row[x] + f(x,y))",
                   "A library without the feature lacks the two symbols"):
        assert phrase in hdr_text, phrase
    assert C.sizeof(wire.EnvironmentDesc) == 40 and C.sizeof(wire.EnvironmentInfo) == 8


def test_cpp_restatement_equals_the_host_statements(pinned):
    assert sorted(pinned) == CASE_NAMES
    # the images do what they are planted for
    t = host_tables("black_3x5")
    assert np.array_equal(t[:3], np.full(3, F32(1) / F32(3)))  # marginal fallback
    img = cases()["planted_17x33"]
    h, w = img.shape[:2]
    tables = host_tables("planted_17x33")
    row_pdf = tables[h : h + h * w].reshape(h, w)
    for y in (1, 3, 9, 10):  # black rows and the negative row: the row fallback
        assert np.array_equal(row_pdf[y], np.full(w, F32(1) / F32(w))), y
    assert abs(float(row_pdf[5, w // 2]) - 1) < 1e-6 and np.count_nonzero(row_pdf[5]) == 1  # a single lit texel
    row_cdf = tables[h + h * w + h + 1 :].reshape(h, w + 1)
    assert np.all(row_pdf[7] > 0) and np.all(np.diff(row_cdf[7]) > 0)  # subnormals: the row sums to something positive and is not the fallback
    assert 0 < float(np.abs(img[7, :, :3]).max()) < np.finfo(F32).tiny
    # a NaN texel makes its row's integral a NaN: the row takes the fallback and no NaN reaches the tables; the mip chain carries it
    nan_pdf = host_tables("nan_17x33")[h : h + h * w].reshape(h, w)
    assert not np.isnan(host_tables("nan_17x33")).any() and np.array_equal(nan_pdf[17 // 2], np.full(w, F32(1) / F32(w)))
    assert all(np.isnan(lv).any() for lv in host_mips("nan_17x33"))
    # a +inf texel makes the integral +inf, which is > 0: inf / inf stands in the row's tables and in the marginal's
    assert np.isnan(host_tables("inf_17x33")).any() and np.isnan(host_tables("inf_65x129")).any()
    assert not np.isnan(host_tables("planted_130x257")).any()


def test_cpp_restatement_under_sanitizers(tmp_path):
    exe = str(tmp_path / "environment_ref_san")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-o", exe, REF_SRC])
    for name in ("planted_1x1", "planted_2x1", "planted_17x33", "nan_17x33", "black_3x5"):
        assert same(run_ref(exe, str(tmp_path), "tables", cases()[name]), host_tables(name)), name
        assert run_ref(exe, str(tmp_path), "mips", cases()[name]).size == sum(lv.size for lv in host_mips(name))


def test_refusals_and_accepted_descriptions_on_the_host_under_sanitizers(tmp_path):
    """tests/cpp/environment_check.cpp links scene_prepare.cpp only: every refusal of the header returns its code and message,
    every accepted description passes, under -fsanitize=address,undefined."""
    exe = str(tmp_path / "environment_check")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-o", exe, CHECK_SRC,
                           os.path.join(ROOT, "stratum_amd", "csrc", "scene_prepare.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ENVIRONMENT CHECK OK" in out.stdout and "FAIL" not in out.stdout, out.stdout + out.stderr
    for case in ("no scene", "struct_size", "unaligned address", "pixels for a record without an image", "wrong width", "table outside gDistributions", "overlapping tables", "zero value",
                 "8-bit environment, pixels", "pixels for an image a material names", "tables only", "value only"):
        assert re.search(r"^ok\s+%s" % re.escape(case), out.stdout, re.M), case


def sky_scene(image, value=(1.0, 1.0, 1.0), tables="host", share=False):
    """An emissive quad over a diffuse floor under the image environment. The floor has the identity transform (part of the
    merged world-space mesh), the lamp has not. share: the floor's base colour image is the environment's image."""
    b = SceneBuilder("sky")
    floor = b.add_material((0.6, 0.6, 0.6), roughness=0.7)
    lamp = b.add_emitter((9.0, 7.0, 5.0))
    handle = b.add_image(image)
    if share:
        b.set_material_images(floor, base_color_image=handle)
    S = 3.0
    b.add_instance(b.add_mesh(*scenes._quad((-S, 0, S), (S, 0, S), (S, 0, -S), (-S, 0, -S), (0, 1, 0))), floor)
    b.add_instance(b.add_mesh(*scenes._quad((-0.4, 0, -0.4), (0.4, 0, -0.4), (0.4, 0, 0.4), (-0.4, 0, 0.4), (0, -1, 0))), lamp, translate((0.0, 1.8, 0.0)))
    b.set_environment(value, handle)
    return b.build(environment_tables=tables)


CAM = {"eye": (0.0, 1.2, 5.0), "target": (0.0, 0.7, 0.0), "fovy": np.radians(45.0)}


def test_device_tables_keep_the_offsets_and_the_count():
    img = np.array(cases()["planted_17x33"])
    host, dev = sky_scene(img), sky_scene(img, tables="device")
    assert host.materials.tobytes() == dev.materials.tobytes()  # the record names the same four offsets
    assert host.environment_address == dev.environment_address and host.distributions.size == dev.distributions.size == 17 + 17 * 33 + 18 + 17 * 34
    assert host.distributions.any() and not dev.distributions.any() and dev.distributions.dtype == np.float32
    assert host.environment_tables == "host" and dev.environment_tables == "device"
    assert dev.desc().distribution_count == host.desc().distribution_count
    with pytest.raises(ValueError):
        SceneBuilder("x").build(environment_tables="gpu")


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def make_renderer(flags=(), args=None, options=None):
    from stratum_amd.bdpt import BDPT

    r = BDPT(device=0, args=dict(args or {}, bdptFlag=list(flags)))
    for k, v in (options or {}).items():
        r.set_option(k, v)
    return r


@pytest.fixture(scope="module")
def ctx(built):
    r = make_renderer()
    yield r
    r.close()


def other_image(name):
    """Sky A of a case: other texels of the same extent."""
    h, w = cases()[name].shape[:2]
    return hdr(h, w, 5000 + h * 7 + w)


def resident_matches(r, name, pinned, what):
    tables, levels = pinned[name]
    assert same(r.read_distributions(), tables), (name, what, "tables")
    assert same(r.read_image(0, 0), cases()[name]), (name, what, "level 0")
    for k, want in enumerate(levels):
        assert same(r.read_image(0, k + 1), want), (name, what, "level %d" % (k + 1))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_gpu_replaced_image_gives_the_host_tables_and_mips(ctx, pinned, name):
    """Sky A with host tables is resident; set_environment(image=B): the tables and every mip level are the host's of B. Then
    back to A from the host and to B once more from a device pointer: the same bytes."""
    import torch

    B = np.array(cases()[name])
    A = other_image(name)
    ctx.update(sky_scene(A))
    info = ctx.set_environment(image=B)
    assert info["device_ms"] >= 0 and info["total_ms"] > 0
    resident_matches(ctx, name, pinned, "host pointer")
    from_host = ctx.read_distributions()
    ctx.set_environment(image=A)
    with np.errstate(all="ignore"):
        assert same(ctx.read_distributions(), np.concatenate(build_distributions(A)))
    dev = torch.from_numpy(B).to("cuda:0")
    torch.cuda.synchronize()
    ctx.set_environment(image=dev, device_ptr=True)
    resident_matches(ctx, name, pinned, "device pointer")
    assert same(ctx.read_distributions(), from_host)


@pytest.mark.gpu
@pytest.mark.parametrize("rows_per_wave", [16, 64])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_gpu_tables_only_form(ctx, pinned, name, rows_per_wave):
    """Uploaded with zero-filled tables (environment_tables="device"): BDPT.update has the device build them; both row
    ownerships of k_env_rows give the host's tables."""
    ctx.set_option("env_rows_per_wave", rows_per_wave)
    try:
        sc = sky_scene(np.array(cases()[name]), tables="device")
        assert not sc.distributions.any()
        ctx.update(sc)
        resident_matches(ctx, name, pinned, "tables only, %d rows per wave" % rows_per_wave)
    finally:
        ctx.set_option("env_rows_per_wave", 16)


def copy(out):
    return {k: np.array(v, copy=True) for k, v in out.items() if isinstance(v, np.ndarray)}


def same_frame(got, want, what):
    for k in OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), (what, k)


RENDER_A = hdr(65, 129, 31)
RENDER_B = hdr(65, 129, 32) * F32(40.0)  # (brighter, another sun: frames of A and B differ visibly)
RENDER_B[..., 3] = 1
VALUE = (0.5, 1.25, 2.0)
ARGS = {"maxPathVertices": 4}
COMBINATIONS = {
    "nee": ["nee", "~sampleenvironmentmapdirectly"],  # the dist2d tables
    "nee_direct": ["nee", "sampleenvironmentmapdirectly"],  # the mip descent
    "plain": ["~nee", "~sampleenvironmentmapdirectly"],  # eval alone
}


def frame_4832():
    return camera.Frame(48, 32, CAM["fovy"], CAM["eye"], CAM["target"])


def fresh_frame(sc, flags, seeds=2, options=None, seed_begin=0):
    r = make_renderer(flags, ARGS, options)
    try:
        r.update(sc)
        return copy(r.render(frame_4832(), seed_begin, seeds))
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("combination", sorted(COMBINATIONS))
def test_gpu_render_parity_with_a_fresh_upload(built, combination):
    """After set_environment(B, value) every output is byte-equal to a fresh context that uploaded the scene built with B and
    the value on the host. For the plain combination the radiance is also the oracle's, byte for byte."""
    flags = COMBINATIONS[combination]
    frame = frame_4832()
    r = make_renderer(flags, ARGS)
    try:
        r.update(sky_scene(RENDER_A))
        before = copy(r.render(frame, 0, 2))
        r.set_environment(value=VALUE, image=RENDER_B)
        got = copy(r.render(frame, 0, 2))
        want_scene = sky_scene(RENDER_B, VALUE)
        want = fresh_frame(want_scene, flags)
        same_frame(got, want, combination)
        assert not np.array_equal(got["radiance"], before["radiance"]) and np.isfinite(got["radiance"]).all()
        sky = got["visibility"]["instance_primitive_index"] == wire.MISS
        assert sky.mean() > 0.1 and got["radiance"][sky][:, :3].max() > 0
        # value alone, on top: the frame of a scene built with it
        r.set_environment(value=(2.0, 0.5, 0.25))
        same_frame(copy(r.render(frame, 0, 2)), fresh_frame(sky_scene(RENDER_B, (2.0, 0.5, 0.25)), flags), combination + ", value only")
        if combination == "plain":
            from oracle import oracle_py

            r.set_environment(value=VALUE)
            got = copy(r.render(frame, 0, 2))
            ref = oracle_py.OracleScene(want_scene).render(frame, r.push_constants(frame), r.mSamplingFlags, 0, 2)
            differing = int((got["radiance"].view(np.uint32) != ref["radiance"].view(np.uint32)).any(axis=-1).sum())
            print("oracle: %d differing pixels of %d" % (differing, 48 * 32))
            assert np.array_equal(got["radiance"].view(np.uint8), np.ascontiguousarray(ref["radiance"]).view(np.uint8))
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_kept_first_hits_survive_the_call(built):
    flags = COMBINATIONS["nee"]
    frame = frame_4832()
    r = make_renderer(flags, ARGS, {"reuse_first_hits": 1})
    try:
        r.update(sky_scene(RENDER_A))
        r.render(frame, 0, 1)
        assert r.stats()["rays_primary_packets"] > 0
        r.set_environment(value=VALUE, image=RENDER_B)
        got = copy(r.render(frame, 0, 1))
        assert r.stats()["rays_primary_packets"] == 0
        same_frame(got, fresh_frame(sky_scene(RENDER_B, VALUE), flags, seeds=1), "kept first hits")
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_kept_scene_follows_a_device_pointer(built):
    """set_environment(B) from a device pointer, then a transform update that moves an instance of the merged mesh: the scene is
    built again from the kept copy, which must have fetched B and its tables first."""
    import torch

    flags = COMBINATIONS["nee"]
    frame = frame_4832()
    moved = translate((0.3, -0.2, 0.1))
    r = make_renderer(flags, ARGS)
    try:
        sc = sky_scene(RENDER_A)
        r.update(sc)
        dev = torch.from_numpy(RENDER_B).to("cuda:0")
        torch.cuda.synchronize()
        r.set_environment(image=dev, device_ptr=True)
        rebuilds = r.stats()["full_rebuilds"]
        sc.set_instance_transform(0, moved)
        r.update_transforms(sc)
        assert r.stats()["full_rebuilds"] == rebuilds + 1
        got = copy(r.render(frame, 0, 2))
        want_scene = sky_scene(RENDER_B)
        want_scene.set_instance_transform(0, moved)
        same_frame(got, fresh_frame(want_scene, flags), "after the rebuild")
        with np.errstate(all="ignore"):
            assert same(r.read_distributions(), np.concatenate(build_distributions(RENDER_B)))
        assert same(r.read_image(0, 0), RENDER_B)
        for k, want in enumerate(np_mips(RENDER_B)):
            assert same(r.read_image(0, k + 1), want), k
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_a_frame_in_flight_completes_with_the_environment_before(built):
    flags = COMBINATIONS["nee"]
    frame = frame_4832()
    r = make_renderer(flags, ARGS)
    try:
        r.update(sky_scene(RENDER_A))
        old = copy(r.render(frame, 0, 2))
        ticket = r.render_async(frame, 0, 2)
        r.set_environment(image=RENDER_B)
        same_frame(copy(r.wait(ticket)), old, "the ticket in flight")
        new = copy(r.wait(r.render_async(frame, 0, 2)))
        same_frame(new, fresh_frame(sky_scene(RENDER_B), flags), "the next frame")
        assert not np.array_equal(new["radiance"], old["radiance"])
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_refusals_leave_the_scene_as_it_was(built):
    from stratum_amd import _lib

    flags = COMBINATIONS["nee"]
    frame = frame_4832()
    r = make_renderer(flags, ARGS)
    try:
        with pytest.raises(_lib.StratumHipError, match="no scene"):
            r.set_environment(value=VALUE)
        r.update(sky_scene(RENDER_A))
        before = copy(r.render(frame, 0, 2))
        tables = r.read_distributions()
        with pytest.raises(_lib.StratumHipError, match=r"\(-1\).*extent"):
            r.set_environment(image=hdr(64, 129, 1))
        with pytest.raises(_lib.StratumHipError, match=r"\(-1\).*zero"):
            r.set_environment(value=(0.0, 0.0, 0.0), image=RENDER_B)
        assert np.array_equal(r.read_distributions().view(np.uint32), tables.view(np.uint32)) and same(r.read_image(0, 0), RENDER_A)
        same_frame(copy(r.render(frame, 0, 2)), before, "after the refusals")
        # an image a material shares
        shared = sky_scene(RENDER_A, share=True)
        r.update(shared)
        before = copy(r.render(frame, 0, 2))
        with pytest.raises(_lib.StratumHipError, match=r"\(-4\).*material record"):
            r.set_environment(image=RENDER_B)
        assert same(r.read_image(0, 0), RENDER_A)
        same_frame(copy(r.render(frame, 0, 2)), before, "after the shared image's refusal")
        r.set_environment(value=VALUE)  # (the value of such an environment may change)
        same_frame(copy(r.render(frame, 0, 2)), fresh_frame(sky_scene(RENDER_A, VALUE, share=True), flags), "shared image, new value")
        # an 8-bit environment (render refuses it too)
        bytes_image = np.clip(RENDER_A * 255.0, 0, 255).astype(np.uint8)
        r.update(sky_scene(bytes_image))
        with pytest.raises(_lib.StratumHipError, match=r"\(-4\).*8-bit"):
            r.set_environment(image=RENDER_B)
        with pytest.raises(_lib.StratumHipError, match=r"\(-4\).*8-bit"):
            r.set_environment()
        assert np.array_equal(r.read_image(0, 0), bytes_image)
        r.update(sky_scene(RENDER_A))
        same_frame(copy(r.render(frame, 0, 2)), fresh_frame(sky_scene(RENDER_A), flags), "the context after all of it")
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_render_parity_with_poisoned_allocations(built):
    """The render-parity tests and one tables-only case once more in a fresh child process with STHIP_POISON_ALLOC (read once
    per process): every new device buffer starts as 0x7F bytes. What this adds to the bit comparisons of the tests above is
    small: the image and table arrays were written in full by the upload before the call, so only the call's own scratch (the
    rows' integrals, the sines) starts poisoned, and a pass that read an integral or a sine nobody wrote would show."""
    if os.environ.get("STHIP_ENVIRONMENT_POISON_CHILD"):
        return  # (this is the child)
    env = dict(os.environ, STHIP_POISON_ALLOC="0x7F", STHIP_ENVIRONMENT_POISON_CHILD="1")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "render_parity_with_a_fresh_upload or (tables_only and 17x33)"],
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "failed" not in out.stdout
