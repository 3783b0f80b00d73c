"""Half colour precision (include/sthip.h: "half_color_precision"; the reference's mHalfColorPrecision, BDPT.cpp:231,553-558).

While the option is on, the colour images of sthip_render (radiance, albedo, debug) and of the post calls are RGBA16F. The
arithmetic stays binary32 and an image is rounded to nearest even only where it leaves the library or persists between
frames, so the test oracle is: half output == np.float16(binary32 output of the same call on the upcast inputs), bit for bit.
"""
import os

import numpy as np
import pytest

from stratum_amd import camera, scenes, shard, wire

FLAG_SETS = [(), ("~nee",), ("connecttoviews",), ("connecttolightpaths",), ("neereservoirs", "neereservoirreuse")]


def rtne(a):
    """binary32 -> binary16, round to nearest even (numpy's conversion; det_f32tof16 on the device)."""
    with np.errstate(over="ignore"):  # (beyond 65504: infinity, as on the device)
        return np.asarray(a, np.float32).astype(np.float16)


def assert_half_of(got, want32, what=""):
    """got (float16) holds the RTNE halves of want32 (float32), bit for bit; a NaN only has to be a NaN."""
    assert got.dtype == np.float16, (what, got.dtype)
    want = rtne(want32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    bad = got.view(np.uint16)[~nan] != want.view(np.uint16)[~nan]
    assert not bad.any(), "%s: %d of %d values differ" % (what, int(bad.sum()), bad.size)


def foggy_cornell():
    return scenes.cornell_box(fog=np.load(os.path.join(os.path.dirname(__file__), "golden", "fog_sphere.npz"))["grid"], anisotropy=0.3)


# ---- CPU: the host side of the seed split and the tile mirror ----
def test_seed_split_helpers_refuse_half_images():
    img = np.ones((4, 4, 4), np.float16)
    with pytest.raises(ValueError, match="half colour precision"):
        shard.to_sums(img)
    with pytest.raises(ValueError, match="half colour precision"):
        shard.from_sums(img)
    f = np.ones((4, 4, 4), np.float32)
    assert shard.to_sums(f) is f  # binary32 stays as it was


def test_assemble_tiles_mirror_keeps_half_entries():
    w, h, world, tw, th = 96, 64, 3, 16, 8
    ref = rtne(np.random.RandomState(3).rand(h, w, 4))
    packed = []
    for r in range(world):
        xy = shard.slot_pixels(w, h, r, world, tw, th)
        ok = xy[:, 0] >= 0
        buf = np.zeros((shard.slot_count(w, h, 0, world, tw, th), 4), np.float16)
        buf[: xy.shape[0]][ok] = ref[xy[ok, 1], xy[ok, 0]]
        packed.append(buf)
    got = shard.assemble_tiles(packed, w, h, tw, th)
    assert got.dtype == np.float16 and np.array_equal(got.view(np.uint16), ref.view(np.uint16))


def test_header_documents_the_option():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sthip.h")).read()
    assert '"half_color_precision"' in hdr and "RGBA16F" in hdr


# ---- GPU ----
def _renderer(sc, flags=(), half=False, args=None):
    from stratum_amd.bdpt import BDPT

    a = {"bdptFlag": list(flags)}
    a.update(args or {})
    r = BDPT(device=0, args=a)
    r.update(sc)
    if half:
        r.set_half_color_precision(True)
    return r


def _compare_frames(half, full, what):
    assert_half_of(half["radiance"], full["radiance"], what + " radiance")
    if "albedo" in full:
        assert_half_of(half["albedo"], full["albedo"], what + " albedo")
    for k in ("visibility", "depth", "prev_uv", "ray_count"):
        if k in full:
            assert half[k].dtype == full[k].dtype and np.array_equal(half[k].view(np.uint8), full[k].view(np.uint8)), (what, k)


@pytest.mark.gpu
def test_option_round_trip(built, cornell):
    sc, cam = cornell
    frame = camera.Frame(64, 48, cam["fovy"], cam["eye"], cam["target"])
    r = _renderer(sc)
    fresh = _renderer(sc)
    try:
        from stratum_amd._lib import StratumHipError

        with pytest.raises(StratumHipError):
            r.set_option("half_color_precision", 2)
        r.set_half_color_precision(True)
        assert r.half_color_precision and r.color_dtype == np.float16
        h = r.render(frame, 0, 2)
        assert h["radiance"].dtype == np.float16 and h["radiance"].shape == (48, 64, 4) and h["albedo"].dtype == np.float16
        r.set_half_color_precision(False)
        back = r.render(frame, 0, 2)
        want = fresh.render(frame, 0, 2)
        for k in want:
            assert want[k].dtype == back[k].dtype and np.array_equal(back[k].view(np.uint8), want[k].view(np.uint8)), k
        _compare_frames(h, want, "half")
    finally:
        r.close()
        fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", FLAG_SETS, ids=lambda f: "+".join(f) or "default")
def test_render_half_is_rtne_of_binary32(built, cornell, flags):
    """Cornell box 256x256, 3 seeds: host pointers, then device pointers (torch float16 buffers)."""
    import torch

    sc, cam = cornell
    frame = camera.Frame(256, 256, cam["fovy"], cam["eye"], cam["target"])
    args = {"maxDiffuseVertices": 3} if "connecttolightpaths" in flags else None
    full_r = _renderer(sc, flags, args=args)
    half_r = _renderer(sc, flags, half=True, args=args)
    try:
        full = full_r.render(frame, 0, 3)
        half = half_r.render(frame, 0, 3)
        _compare_frames(half, full, "host")
        W, H = frame.width, frame.height
        dev = {
            "radiance": torch.zeros((H, W, 4), dtype=torch.float16, device="cuda"),
            "albedo": torch.zeros((H, W, 4), dtype=torch.float16, device="cuda"),
            "visibility": torch.zeros((H, W, 2), dtype=torch.int32, device="cuda"),
            "ray_count": torch.zeros(2, dtype=torch.int64, device="cuda"),
        }
        torch.cuda.synchronize()
        half_r.render(frame, 0, 3, device_outputs={k: v.data_ptr() for k, v in dev.items()})
        half_r.stats()  # joins the context's stream
        torch.cuda.synchronize()
        assert_half_of(dev["radiance"].cpu().numpy(), full["radiance"], "device radiance")
        assert_half_of(dev["albedo"].cpu().numpy(), full["albedo"], "device albedo")
        assert np.array_equal(dev["visibility"].cpu().numpy().view(np.uint8).ravel(), full["visibility"].view(np.uint8).ravel())
        assert np.array_equal(dev["ray_count"].cpu().numpy().view(np.uint64), full["ray_count"])
    finally:
        full_r.close()
        half_r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [(), ("~nee",)], ids=lambda f: "+".join(f) or "default")
def test_render_half_fogged_box(built, flags):
    sc, cam = foggy_cornell()
    frame = camera.Frame(128, 128, cam["fovy"], cam["eye"], cam["target"])
    full_r, half_r = _renderer(sc, flags), _renderer(sc, flags, half=True)
    try:
        _compare_frames(half_r.render(frame, 0, 3), full_r.render(frame, 0, 3), "fog")
    finally:
        full_r.close()
        half_r.close()


@pytest.mark.gpu
def test_render_half_against_the_oracle(built, cornell):
    from oracle import oracle_py

    sc, cam = cornell
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    r = _renderer(sc, half=True)
    try:
        got = r.render(frame, 0, 2)
        ref = oracle_py.OracleScene(sc).render(frame, r.push_constants(frame), r.mSamplingFlags, 0, 2)
        _compare_frames(got, ref, "oracle")
    finally:
        r.close()


def _debug_args(mode):
    flags, view_length, light_length = (), 0, 0
    if mode == wire.DEBUG_LIGHT_TRACE_CONTRIBUTION:
        flags = ("connecttoviews",)
    if mode == wire.DEBUG_PATH_LENGTH_CONTRIBUTION:
        flags, view_length, light_length = ("connecttoviews",), 1, 2
    if mode == wire.DEBUG_RESERVOIR_WEIGHT:
        flags = ("neereservoirs", "~defershadowrays")
    return flags, view_length, light_length


@pytest.mark.gpu
@pytest.mark.parametrize("mode", range(1, wire.DEBUG_MODE_COUNT))
def test_debug_image_half(built, cornell, mode):
    """A 3-seed half call equals three chained 1-seed half calls; each 1-seed half call equals RTNE of the binary32 call given
    the upcast half image."""
    sc, cam = cornell
    if mode in (wire.DEBUG_ENVIRONMENT_SAMPLE_TEST, wire.DEBUG_ENVIRONMENT_SAMPLE_PDF):  # (they sample the environment)
        sc, cam = scenes.environment_scene(image=True, emitter=True)
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    flags, vl, ll = _debug_args(mode)
    full_r, half_r = _renderer(sc, flags), _renderer(sc, flags, half=True)
    try:
        for r in (full_r, half_r):
            r.mPushConstants.gDebugViewPathLength = vl
            r.mPushConstants.gDebugLightPathLength = ll
        start = rtne(np.random.RandomState(mode).rand(64, 96, 4) * 0.5)
        three = half_r.render(frame, 0, 3, debug_mode=mode, debug_image=start)
        img = start
        for seed in range(3):
            one = half_r.render(frame, seed, 1, debug_mode=mode, debug_image=img)
            ref = full_r.render(frame, seed, 1, debug_mode=mode, debug_image=img.astype(np.float32))
            assert_half_of(one["debug"], ref["debug"], "mode %d seed %d debug" % (mode, seed))
            assert_half_of(one["radiance"], ref["radiance"], "mode %d seed %d radiance" % (mode, seed))
            img = one["debug"]
        assert np.array_equal(three["debug"].view(np.uint16), img.view(np.uint16)), mode
    finally:
        full_r.close()
        half_r.close()


@pytest.mark.gpu
def test_tile_shards_half(built, cornell):
    """8 ranks on one GPU render packed half tiles; sthip_assemble_tiles gives the unsharded half frame bit for bit, and
    sthip_pack_tiles / sthip_assemble_tiles_bytes do the same for the 8-byte albedo."""
    import torch

    sc, cam = cornell
    W, H = 256, 192
    frame = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
    r = _renderer(sc, half=True)
    try:
        whole = r.render(frame, 0, 2)
        world, tw, th = 8, 32, 16
        r.set_shard(0, world, tw, th)
        stride = r.shard_slot_count(frame, 0)
        gathered = torch.zeros((world, stride, 4), dtype=torch.float16, device="cuda")
        gathered_alb = torch.zeros((world, stride, 4), dtype=torch.float16, device="cuda")
        for rank in range(world):
            r.set_shard(rank, world, tw, th)
            alb = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
            torch.cuda.synchronize()
            r.render(frame, 0, 2, device_outputs={"radiance": gathered[rank].data_ptr(), "albedo": alb.data_ptr()}, packed_tiles=True)
            r.pack_tiles(frame, alb.data_ptr(), 8, gathered_alb[rank].data_ptr())
            r.stats()
            torch.cuda.synchronize()
        img = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
        img_alb = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
        r.assemble_tiles(frame, gathered.data_ptr(), stride, img.data_ptr())
        r.assemble_tiles_bytes(frame, gathered_alb.data_ptr(), stride, img_alb.data_ptr(), 8)
        r.stats()
        torch.cuda.synchronize()
        assert np.array_equal(img.cpu().numpy().view(np.uint16), whole["radiance"].view(np.uint16))
        assert np.array_equal(img_alb.cpu().numpy().view(np.uint16), whole["albedo"].view(np.uint16))
    finally:
        r.close()


@pytest.mark.gpu
def test_seed_split_refused_under_half(built, cornell):
    import torch

    from stratum_amd._lib import StratumHipError

    sc, cam = cornell
    frame = camera.Frame(64, 32, cam["fovy"], cam["eye"], cam["target"])
    r = _renderer(sc, half=True)
    try:
        buf = torch.zeros((32, 64, 4), dtype=torch.float16, device="cuda")
        with pytest.raises(StratumHipError, match="half_color_precision"):
            r.radiance_to_sums(buf.data_ptr(), 32 * 64)
        got = r.render(frame, 0, 1)  # the context still renders
        assert got["radiance"].dtype == np.float16 and np.isfinite(got["radiance"]).all() and (got["radiance"][..., 3] == 1).all()
    finally:
        r.close()


def _post_pair():
    from stratum_amd.bdpt import BDPT

    full, half = BDPT(device=0), BDPT(device=0)
    half.set_half_color_precision(True)
    return full, half


def _hdr_half(h, w, seed):
    rs = np.random.RandomState(seed)
    img = rtne(np.exp(rs.randn(h, w, 4) * 2.0) * (rs.rand(h, w, 4) < 0.97))
    img[..., 3] = 1
    img[3, 4, 1] = np.nan
    alb = rtne(rs.rand(h, w, 4))
    return img, alb


@pytest.mark.gpu
def test_post_tonemap_half(built, cornell):
    from stratum_amd.post import Tonemapper

    full, half = _post_pair()
    try:
        img, alb = _hdr_half(61, 83, 7)
        for mode in wire.TONEMAP_MODES:
            for modulate in (False, True):
                for gamma in (False, True):
                    tf = Tonemapper(full, mode, 0.7, gamma, exposure_alpha=0.4)
                    th = Tonemapper(half, mode, 0.7, gamma, exposure_alpha=0.4)
                    for k in range(3):
                        fi, hi = img * np.float16(1 + k), img * np.float16(1 + k)
                        wf, mf = tf(fi.astype(np.float32), alb.astype(np.float32), modulate_albedo=modulate, return_max=True)
                        wh, mh = th(hi, alb, modulate_albedo=modulate, return_max=True)
                        what = "%s modulate=%d gamma=%d frame %d" % (mode, modulate, gamma, k)
                        assert_half_of(wh, wf, what)
                        assert np.array_equal(mf.view(np.uint32), mh.view(np.uint32)), what
                        assert np.array_equal(tf.state.view(np.uint32), th.state.view(np.uint32)), what
    finally:
        full.close()
        half.close()


@pytest.mark.gpu
@pytest.mark.parametrize("reprojection,demodulate,limit", [(False, False, 0.0), (True, False, 0.0), (True, True, 2.0), (False, True, 0.0)])
def test_post_accumulate_half(built, cornell, reprojection, demodulate, limit):
    from stratum_amd.post import TemporalAccumulation

    sc, cam = cornell
    full, half = _post_pair()
    half.update(sc)
    try:
        fa = TemporalAccumulation(full, reprojection, demodulate, limit)
        ha = TemporalAccumulation(half, reprojection, demodulate, limit)
        prev = None
        for k in range(3):
            eye = np.array(cam["eye"]) + np.array([0.05, 0.02, 0.0]) * k
            fr = camera.Frame(96, 64, cam["fovy"], tuple(eye), cam["target"], prev=prev)
            out = half.render(fr, k, 1)
            up = dict(out, radiance=out["radiance"].astype(np.float32), albedo=out["albedo"].astype(np.float32))
            if ha.history is not None:  # the binary32 run continues from the upcast half history
                fa.history = dict(ha.history, accum_color=ha.history["accum_color"].astype(np.float32))
            fc, fm = fa(up, fr.views)
            hc, hm = ha(out, fr.views)
            assert_half_of(hc, fc, "frame %d colour" % k)
            assert np.array_equal(hm.view(np.uint32), fm.view(np.uint32)), k
            prev = fr
        assert hc[..., 3].max() == (limit if limit else 3)
    finally:
        full.close()
        half.close()


@pytest.mark.gpu
def test_post_image_compare_half(built, cornell):
    from stratum_amd.post import ImageComparer

    full, half = _post_pair()
    try:
        a, _ = _hdr_half(53, 71, 1)
        b, _ = _hdr_half(53, 71, 2)
        a, b = np.abs(np.nan_to_num(a, nan=0.5)), np.abs(np.nan_to_num(b, nan=0.5))
        for metric in wire.COMPARE_MODES:
            want = ImageComparer(full, metric).raw(a.astype(np.float32), b.astype(np.float32))
            got = ImageComparer(half, metric).raw(a, b)
            assert got == want, metric
    finally:
        full.close()
        half.close()


# ---- the C++ host (stratum_amd/host): tests/cpp/half_host.cpp ----
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile_half_host(exe):
    """The driver, -Wall -Werror against the host headers; links the library, RCCL and the HIP runtime (as build_multi_host)."""
    import subprocess

    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    lib = os.path.join(ROOT, "stratum_amd")
    subprocess.check_call(
        ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "half_host.cpp")]
        + ["-L" + lib, "-lstratum_hip", "-L" + os.path.join(rocm, "lib"), "-lrccl", "-lamdhip64", "-lpthread", "-Wl,-rpath," + lib, "-Wl,-rpath," + os.path.join(rocm, "lib")]
    )
    return exe


@pytest.fixture(scope="module")
def half_host(built, tmp_path_factory):
    return _compile_half_host(str(tmp_path_factory.mktemp("half_host") / "half_host"))


def test_half_host_driver_compiles(half_host):
    assert os.path.exists(half_host)


@pytest.mark.gpu
def test_cpp_host_half_frame(half_host, tmp_path, cornell):
    """BDPT with the switch on: mRadiance16 / mTonemapResult16 are the Python host's half outputs, export_hdr writes what
    sthip_write_hdr writes of the upcast image, and MultiDeviceBDPT at world 1 (tile mode) gives the single-device half frame."""
    import subprocess

    from stratum_amd.bdpt import BDPT
    from stratum_amd.post import Tonemapper, write_hdr
    from stratum_amd.scene import dump_description

    sc, cam = cornell
    W, H, seeds = 96, 64, 3
    fr = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
    desc, outp, hdr = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin"), str(tmp_path / "image.hdr")
    dump_description(desc, sc, fr)
    out = subprocess.run([half_host, "render", desc, outp, str(seeds), str(wire.TONEMAP["ACES"]), "0.75", hdr], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("HALF RENDER OK"), out.stdout + out.stderr
    raw = np.fromfile(outp, dtype=np.float16)
    rad, tm = raw[: W * H * 4].reshape(H, W, 4), raw[W * H * 4 :].reshape(H, W, 4)
    r = BDPT(device=0)
    try:
        r.update(sc)
        r.set_half_color_precision(True)
        ref = r.render(fr, 0, seeds)
        ref_tm = Tonemapper(r, "ACES", 0.75, True)(ref["radiance"])
    finally:
        r.close()
    assert np.array_equal(rad.view(np.uint16), ref["radiance"].view(np.uint16))
    assert np.array_equal(tm.view(np.uint16), ref_tm.view(np.uint16))
    write_hdr(tmp_path / "py.hdr", ref["radiance"].astype(np.float32))
    assert open(hdr, "rb").read() == (tmp_path / "py.hdr").read_bytes()
    # the multi-GPU host at world 1: packed 8-byte tiles through the gather and sthip_assemble_tiles
    outm = str(tmp_path / "multi.bin")
    out = subprocess.run([half_host, "multi", desc, outm, str(seeds), "0"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "seed split refused" in out.stdout, out.stdout + out.stderr
    raw = np.fromfile(outm, dtype=np.float16)
    assert np.array_equal(raw[: W * H * 4].view(np.uint16), ref["radiance"].view(np.uint16).ravel())
    assert np.array_equal(raw[W * H * 4 :].view(np.uint16), ref["albedo"].view(np.uint16).ravel())
