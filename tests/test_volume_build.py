"""Density grids from dense voxel arrays, built on the device (include/sthip.h: sthip_build_volume; csrc/volume_build.hip):
byte for byte the numpy statement's buffer (stratum_amd/nvdb.py, which tests/test_nvdb_build.py pins against the fixture and
the oracle's reader) from host and device pointers into host and device outputs, its refusals, and frames of the fog Cornell
box with the device-built grid."""
import ctypes as C
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
from stratum_amd import camera, nvdb, scenes, wire  # noqa: E402

F32 = np.float32
INVALID = -1  # STHIP_ERR_INVALID_ARGUMENT
POISON = 0x7F
OUTPUTS = ("radiance", "albedo", "visibility", "depth", "prev_uv", "ray_count")


def make_renderer(flags=(), args=None):
    from stratum_amd.bdpt import BDPT

    return BDPT(device=0, args=dict(args or {}, bdptFlag=list(flags)))


def last_error(r):
    from stratum_amd import _lib

    return _lib.lib().sthip_last_error(r._h).decode()


def desc_of(dense_ptr, is_device, dims, origin, voxel, tr, name):
    d = wire.DenseVolumeDesc()
    d.struct_size, d.dense, d.dense_is_device, d.voxel_size = C.sizeof(wire.DenseVolumeDesc), dense_ptr, int(is_device), float(voxel)
    for k in range(3):
        d.dims[k], d.origin[k], d.translation[k] = int(dims[k]), int(origin[k]), float(tr[k])
    d.name = name.encode() if name is not None else None
    return d


def test_header_declares_the_call():
    import re

    text = open(os.path.join(ROOT, "include", "sthip.h")).read()
    assert re.search(r"int\s+sthip_build_volume\s*\(\s*sthip_ctx\s*\*\s*\w+\s*,\s*const\s+sthip_dense_volume_desc\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*,\s*uint64_t\s+\w+\s*,\s*int\s+\w+\s*,\s*sthip_volume_info\s*\*\s*\w+\s*\)", text)
    assert re.search(r"int\s+sthip_scene_set_volume\s*\(\s*sthip_ctx\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*const\s+sthip_volume_source\s*\*\s*\w+\s*,\s*sthip_volume_info\s*\*\s*\w+\s*\)", text)
    assert re.search(r"int\s+sthip_scene_read_volume\s*\(\s*sthip_ctx\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*void\s*\*\s*\w+\s*,\s*uint64_t\s+\w+\s*,\s*uint64_t\s*\*\s*\w+\s*\)", text)
    from stratum_amd import _lib

    assert {"sthip_build_volume", "sthip_scene_set_volume", "sthip_scene_read_volume"} <= set(_lib.EXPORTS)


def test_wire_structs_equal_the_header(built, tmp_path):
    """sizeof and every offset of the two structs, from a C program that includes the header."""
    fields = {"sthip_dense_volume_desc": ["struct_size", "dense_is_device", "dense", "dims", "origin", "voxel_size", "translation", "name"],
              "sthip_volume_info": ["bytes", "bbox_min", "bbox_max", "world_bbox", "min", "max", "active_voxels", "leaf_count", "lower_count", "upper_count", "root_tiles", "device_ms", "call_ms"]}
    src, exe = tmp_path / "layout.c", str(tmp_path / "layout")
    body = "".join('printf("%%zu", sizeof(%s));%s printf("\\n");' % (s, "".join(' printf(" %%zu", offsetof(%s, %s));' % (s, f) for f in fs)) for s, fs in fields.items())
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sthip.h"\nint main(void) { %s return 0; }\n' % body)
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    lines = subprocess.check_output([exe], text=True).strip().split("\n")
    for line, (s, fs), T in zip(lines, fields.items(), (wire.DenseVolumeDesc, wire.VolumeInfo)):
        assert [int(x) for x in line.split()] == [C.sizeof(T)] + [getattr(T, f).offset for f in fs], s


def check_info(info, grid, what):
    want = nvdb.grid_info(grid)
    assert info["bytes"] == want["bytes"] and list(info["bbox_min"]) == list(want["bbox_min"]) and list(info["bbox_max"]) == list(want["bbox_max"]), what
    assert np.array_equal(np.asarray(info["world_bbox"]), want["world_bbox"]), what
    assert F32(info["min"]) == F32(want["min"]) and F32(info["max"]) == F32(want["max"]) and info["active_voxels"] == want["active_voxels"], what
    assert (info["leaf_count"], info["lower_count"], info["upper_count"], info["root_tiles"]) == (want["leaf_count"], want["lower_count"], want["upper_count"], want["root_tiles"]), what
    assert info["device_ms"] > 0 and info["call_ms"] > 0, what


@pytest.mark.gpu
@pytest.mark.parametrize("name", vc.ALL)
def test_gpu_build_volume_equals_the_numpy_statement(built, name):
    """From a host pointer and a device pointer, into host and device outputs, twice in a row: byte for byte the numpy
    statement's buffer. The device output starts as 0x7F bytes, so padding nobody wrote shows; a device box that is 4 bytes off
    a 16-byte boundary takes the per-element loads. The two-call capacity idiom."""
    import torch

    from stratum_amd import _lib

    L = _lib.lib()
    dense, origin, voxel, tr, nm = vc.case(name)
    want = vc.numpy_grid(name)
    r = make_renderer()
    try:
        dev = torch.from_numpy(np.array(dense)).to("cuda:0")
        shifted = torch.zeros(dense.size + 1, dtype=torch.float32, device="cuda:0")
        shifted[1:] = dev.reshape(-1)
        torch.cuda.synchronize()
        for rep in range(2):
            grid, info = r.build_volume(np.array(dense), origin, voxel, tr, nm)  # host -> host
            assert np.array_equal(grid, want), ("host to host", rep, np.flatnonzero(grid != want)[:8])
            check_info(info, want, "host to host")
            grid, info = r.build_volume(dev.data_ptr(), origin, voxel, tr, nm, dims=dense.shape)  # device -> host
            assert np.array_equal(grid, want), ("device to host", rep, np.flatnonzero(grid != want)[:8])
            for source, what in ((np.array(dense), "host to device"), (dev.data_ptr(), "device to device"), (shifted.data_ptr() + 4, "misaligned device to device")):
                out = torch.full((want.size + 64,), POISON, dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                _, info = r.build_volume(source, origin, voxel, tr, nm, dims=dense.shape, out=out.data_ptr(), capacity=out.numel())
                got = out.cpu().numpy()
                assert np.array_equal(got[: want.size], want), (what, rep, np.flatnonzero(got[: want.size] != want)[:8])
                assert (got[want.size :] == POISON).all(), what  # nothing behind the grid is written
                check_info(info, want, what)
        # a capacity that is too small: the size comes back, nothing is written, the call is refused
        small = np.full(want.size, POISON, np.uint8)
        info = wire.VolumeInfo()
        host_dense = np.array(dense)
        d = desc_of(host_dense.ctypes.data, 0, dense.shape, origin, voxel, tr, nm)
        assert L.sthip_build_volume(r._h, C.byref(d), wire.ptr(small), want.size - 1, 0, C.byref(info)) == INVALID
        assert info.bytes == want.size and (small == POISON).all() and "capacity" in last_error(r)
        out = torch.full((want.size,), POISON, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert L.sthip_build_volume(r._h, C.byref(d), C.c_void_p(out.data_ptr()), want.size - 4, 1, C.byref(info)) == INVALID
        assert info.bytes == want.size and bool((out == POISON).all())
        assert L.sthip_build_volume(r._h, C.byref(d), wire.ptr(small), want.size, 0, C.byref(info)) == 0 and np.array_equal(small, want)
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_build_volume_refusals(built):
    """Every refusal leaves the output buffer and the info untouched and names its reason."""
    from stratum_amd import _lib

    L = _lib.lib()
    ok = np.ones((3, 4, 5), F32)
    nan, inf, neg_inf, zero = ok.copy(), ok.copy(), ok.copy(), np.zeros((9, 9, 9), F32)
    nan[2, 3, 4], inf[0, 0, 0], neg_inf[1, 2, 3] = np.nan, np.inf, -np.inf
    zero[4, 4, 4] = -0.0
    cases = [
        (nan, {}, "NaN"), (inf, {}, "infinite"), (neg_inf, {}, "infinite"), (zero, {}, "no active voxel"),
        (ok, {"voxel": 0.0}, "voxel_size"), (ok, {"voxel": -0.5}, "voxel_size"), (ok, {"voxel": float("inf")}, "voxel_size"), (ok, {"voxel": float("nan")}, "voxel_size"),
        (ok, {"origin": (0, 2**31 - 3, 0)}, "int32"), (ok, {"tr": (0.0, float("nan"), 0.0)}, "translation"), (ok, {"name": "x" * 256}, "name"),
        (ok, {"dims": (3, 0, 5)}, "dims"), (ok, {"struct_size": 72}, "struct_size"),
    ]
    r = make_renderer()
    try:
        for dense, kw, reason in cases:
            out = np.full(1 << 20, POISON, np.uint8)
            info = wire.VolumeInfo()
            C.memset(C.byref(info), POISON, C.sizeof(info))
            d = desc_of(dense.ctypes.data, 0, kw.get("dims", dense.shape), kw.get("origin", (0, 0, 0)), kw.get("voxel", 1.0), kw.get("tr", (0.0, 0.0, 0.0)), kw.get("name", "density"))
            d.struct_size = kw.get("struct_size", d.struct_size)
            assert L.sthip_build_volume(r._h, C.byref(d), wire.ptr(out), out.size, 0, C.byref(info)) == INVALID, reason
            assert reason in last_error(r) and "sthip_build_volume" in last_error(r), (reason, last_error(r))
            assert (out == POISON).all() and bytes(info) == bytes([POISON]) * C.sizeof(info), reason
        d = desc_of(ok.ctypes.data, 0, ok.shape, (0, 0, 0), 1.0, (0.0, 0.0, 0.0), None)
        info = wire.VolumeInfo()
        assert L.sthip_build_volume(r._h, None, None, 0, 0, C.byref(info)) == INVALID and L.sthip_build_volume(r._h, C.byref(d), None, 0, 0, None) == INVALID
        import torch

        out = torch.full((1 << 16,), POISON, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert L.sthip_build_volume(r._h, C.byref(d), C.c_void_p(out.data_ptr() + 8), 1 << 15, 1, C.byref(info)) == INVALID and "aligned" in last_error(r)
        assert bool((out == POISON).all())
        # ... and the same description is accepted once its defect is gone (no name: an empty one)
        grid, _ = r.build_volume(ok, name="")
        assert np.array_equal(grid, nvdb.dense_to_nanovdb(ok, name=""))
    finally:
        r.close()


def frame_copy(out):
    return {k: np.array(v, copy=True) for k, v in out.items() if isinstance(v, np.ndarray)}


def same_frame(got, want, what):
    for k in OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("flags,args", [([], {"maxDiffuseVertices": 3}), (["~defershadowrays"], {"maxDiffuseVertices": 3})], ids=["default", "inline_walks"])
def test_gpu_frames_with_the_device_built_grid(built, flags, args):
    """The fog Cornell box at 64 x 64, two seeds: the upload with the fixture's bytes == the upload with the bytes the device
    built from the fixture's values == the oracle on the numpy statement's bytes, bit for bit."""
    from oracle import oracle_py

    dense, origin, voxel, tr, nm = vc.case("fixture")
    r = make_renderer(flags, args)
    try:
        built_grid, _ = r.build_volume(np.array(dense), origin, voxel, tr, nm)
        assert np.array_equal(built_grid, vc.numpy_grid("fixture"))
        frames = []
        for grid in (vc.fixture()["grid"], built_grid):
            sc, cam = scenes.cornell_box(fog=grid)
            frame = camera.Frame(64, 64, cam["fovy"], cam["eye"], cam["target"])
            r.update(sc)
            frames.append(frame_copy(r.render(frame, 0, 2)))
        same_frame(frames[1], frames[0], "device-built grid against the fixture")
        in_fog = (frames[1]["visibility"]["instance_primitive_index"] & 0xFFFF) == sc.instances.shape[0] - 1
        assert in_fog.mean() > 0.01
        sc, cam = scenes.cornell_box(fog=vc.numpy_grid("fixture"))
        ref = oracle_py.OracleScene(sc).render(frame, r.push_constants(frame), r.mSamplingFlags, 0, 2)
        differing = int((frames[1]["radiance"].view(np.uint32) != np.ascontiguousarray(ref["radiance"]).view(np.uint32)).any(axis=-1).sum())
        print("%s: %d of %d radiance pixels differ from the oracle" % (flags, differing, 64 * 64))
        assert np.array_equal(frames[1]["radiance"].view(np.uint8), np.ascontiguousarray(ref["radiance"]).view(np.uint8))
        assert np.array_equal(frames[1]["ray_count"], ref["ray_count"])
        assert np.array_equal(frames[1]["visibility"]["instance_primitive_index"], ref["visibility"]["instance_primitive_index"])
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_build_volume_with_poisoned_allocations(built):
    """Every byte-for-byte case and one set_volume case once more in a fresh child process with STHIP_POISON_ALLOC (read once per
    process): the build's scratch, its staging area and the grids' new words start as 0x7F bytes, so a record or a byte of a
    grid nobody wrote shows."""
    if os.environ.get("STHIP_VOLUME_POISON_CHILD"):
        return  # (this is the child)
    env = dict(os.environ, STHIP_POISON_ALLOC="0x7F", STHIP_VOLUME_POISON_CHILD="1")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "numpy_statement or (set_volume_equals and four_wide)"], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "failed" not in out.stdout


# ---------------------------------------------------------------------------------------------------------------------------
# sthip_scene_set_volume / sthip_scene_read_volume: the grid of a resident scene
# ---------------------------------------------------------------------------------------------------------------------------
ARGS = {"maxDiffuseVertices": 3}


def small_case():
    """The 13 x 9 x 21 box at voxel size 0.05, translated into the Cornell box (its origin lies at z = 4090)."""
    dense, origin, _, _, nm = vc.case("cropped")
    return np.array(dense), origin, 0.05, (0.0, -0.4, -205.0), nm


def small_grid():
    return nvdb.dense_to_nanovdb(*small_case())


def frame_64(cam):
    return camera.Frame(64, 64, cam["fovy"], cam["eye"], cam["target"])


def renderer_with(flags, options):
    r = make_renderer(flags, ARGS)
    for k, v in (options or {}).items():
        r.set_option(k, v)
    return r


def fresh(sc, cam, flags=(), options=None, seed_begin=0, seeds=2):
    r = renderer_with(flags, options)
    try:
        r.update(sc)
        return frame_copy(r.render(frame_64(cam), seed_begin, seeds))
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [1, 0], ids=["keep_scene", "no_kept_scene"])
@pytest.mark.parametrize("wide", [1, 3], ids=["four_wide", "eight_wide"])
def test_gpu_set_volume_equals_a_fresh_upload(built, wide, keep):
    """Resident with the fixture, set to the small grid from dense device memory, from finished host bytes and from finished
    device bytes: each frame equals a fresh upload of that scene bit for bit, read_volume returns the built bytes, setting the
    fixture back gives the first frame again. With keep_scene a moved instance of the merged mesh then forces the rebuild from
    the kept copy, which must fetch the device-built grid first; without it that move is refused and nothing changes."""
    import torch

    from stratum_amd import _lib
    from stratum_amd.scene import translate

    options = {"wide_bvh": wide, "keep_scene": keep}
    fixture, want_small = vc.fixture()["grid"], small_grid()
    dense, origin, voxel, tr, nm = small_case()
    sc, cam = scenes.cornell_box(fog=fixture)
    small_sc, _ = scenes.cornell_box(fog=want_small)
    first, small = fresh(sc, cam, options=options), fresh(small_sc, cam, options=options)
    assert not np.array_equal(first["radiance"], small["radiance"])
    r = renderer_with((), options)
    try:
        r.update(sc)
        same_frame(frame_copy(r.render(frame_64(cam), 0, 2)), first, "before")
        dev = torch.from_numpy(dense).to("cuda:0")
        dev_grid = torch.from_numpy(np.array(want_small)).to("cuda:0")
        torch.cuda.synchronize()
        info = r.set_volume(0, dense=dev, origin=origin, voxel_size=voxel, translation=tr, name=nm, dims=dense.shape)
        check_info(info, want_small, "set_volume from dense device memory")
        assert np.array_equal(r.read_volume(0), want_small)
        same_frame(frame_copy(r.render(frame_64(cam), 0, 2)), small, "dense device memory")
        r.set_volume(0, grid=fixture)
        assert np.array_equal(r.read_volume(0), fixture)
        same_frame(frame_copy(r.render(frame_64(cam), 0, 2)), first, "set back")
        info = r.set_volume(0, grid=want_small)
        assert info["bytes"] == want_small.size and list(info["bbox_min"]) == list(nvdb.grid_info(want_small)["bbox_min"])
        same_frame(frame_copy(r.render(frame_64(cam), 0, 2)), small, "finished host bytes")
        r.set_volume(0, grid=fixture)
        r.set_volume(0, grid=dev_grid, grid_bytes=want_small.size)
        assert np.array_equal(r.read_volume(0), want_small)
        same_frame(frame_copy(r.render(frame_64(cam), 0, 2)), small, "finished device bytes")
        # a moved instance of the merged mesh: the scene is built again from the kept copy
        moved = translate((0.05, 0.0, -0.05))
        sc.set_instance_transform(0, moved)
        if keep:
            rebuilds = r.stats()["full_rebuilds"]
            r.update_transforms(sc)
            assert r.stats()["full_rebuilds"] == rebuilds + 1
            small_sc.set_instance_transform(0, moved)
            same_frame(frame_copy(r.render(frame_64(cam), 0, 2)), fresh(small_sc, cam, options=options), "after the rebuild from the kept copy")
            assert np.array_equal(r.read_volume(0), want_small)
        else:
            with pytest.raises(_lib.StratumHipError):
                r.update_transforms(sc)
            same_frame(frame_copy(r.render(frame_64(cam), 0, 2)), small, "after the refused move")
        # the scene object handed to update() again first takes the grid that is resident
        sc.set_instance_transform(0, translate((0.0, 0.0, 0.0)))
        r.update(sc)
        assert np.array_equal(sc.volumes[0], want_small)
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_set_volume_refusals_leave_the_resident_frame(built):
    """A finished buffer with a wrong magic or a truncated tile table, a NaN, an all-zero box, a bad voxel size, an index out of
    range, both sources or none: refused with the upload's own words where it has them, and the resident frame stays."""
    from stratum_amd import _lib

    L = _lib.lib()
    fixture = vc.fixture()["grid"]
    sc, cam = scenes.cornell_box(fog=fixture)
    r = renderer_with((), None)
    try:
        r.update(sc)
        first = frame_copy(r.render(frame_64(cam), 0, 2))
        magic = fixture.copy()
        magic[0] ^= 1
        truncated = fixture[: 672 + 64 + 64 + 32 * 4].copy()  # half of the eight tiles
        nan = np.ones((3, 3, 3), F32)
        nan[1, 1, 1] = np.nan
        for kwargs, reason in (
            ({"grid": magic}, "not a NanoVDB float grid"), ({"grid": truncated}, "root tile table lies outside"), ({"grid": fixture[:700].copy()}, "not a NanoVDB float grid"),
            ({"dense": nan}, "NaN"), ({"dense": np.zeros((4, 4, 4), F32)}, "no active voxel"), ({"dense": np.ones((2, 2, 2), F32), "voxel_size": 0.0}, "voxel_size"),
            ({"dense": np.ones((2, 2, 2), F32), "origin": (2**31 - 1, 0, 0)}, "int32"),
        ):
            with pytest.raises(_lib.StratumHipError, match=reason):
                r.set_volume(0, **kwargs)
            assert np.array_equal(r.read_volume(0), fixture), reason
        with pytest.raises(_lib.StratumHipError, match="out of range"):
            r.set_volume(1, grid=fixture)
        s = wire.VolumeSource()
        s.struct_size = C.sizeof(wire.VolumeSource)
        assert L.sthip_scene_set_volume(r._h, 0, C.byref(s), None) == INVALID and "exactly one" in last_error(r)
        s.struct_size = 24
        assert L.sthip_scene_set_volume(r._h, 0, C.byref(s), None) == INVALID and "struct_size" in last_error(r)
        n = C.c_uint64(0)
        small = np.full(16, POISON, np.uint8)
        assert L.sthip_scene_read_volume(r._h, 0, wire.ptr(small), 16, C.byref(n)) == INVALID and n.value == fixture.size and (small == POISON).all()
        same_frame(frame_copy(r.render(frame_64(cam), 0, 2)), first, "after the refusals")
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_set_volume_grows_past_its_slot(built):
    """Two grids, the smaller one first: it is replaced by a larger one, so the second grid's words move. The frame equals a
    fresh upload of the two grids, and the other grid reads back unchanged."""
    from stratum_amd.scene import SceneBuilder, translate

    tiny = vc.numpy_grid("one")
    fixture, want_small = vc.fixture()["grid"], small_grid()
    assert tiny.size < want_small.size

    def scene(first_grid):
        b = SceneBuilder("two_clouds")
        quad = b.add_mesh(*scenes._quad((-1, -1, -1), (1, -1, -1), (1, -1, 1), (-1, -1, 1), (0, 1, 0)))
        b.add_instance(quad, b.add_material((0.7, 0.7, 0.7)))
        top = b.add_mesh(*scenes._quad((-0.5, 1, -0.5), (-0.5, 1, 0.5), (0.5, 1, 0.5), (0.5, 1, -0.5), (0, -1, 0)))
        b.add_instance(top, b.add_emitter((9.0, 9.0, 9.0)))
        b.add_medium(b.add_volume(first_grid), density_scale=(4, 4, 4), albedo_scale=(0.9, 0.9, 0.9), transform=translate((0.0, 0.6, 0.0)))
        b.add_medium(b.add_volume(fixture), density_scale=(3, 3, 3), albedo_scale=(0.9, 0.9, 0.9))
        return b.build()

    cam = scenes.cornell_box()[1]
    dense, origin, voxel, tr, nm = small_case()
    want = fresh(scene(want_small), cam)
    r = renderer_with((), None)
    try:
        r.update(scene(tiny))
        r.set_volume(0, dense=dense, origin=origin, voxel_size=voxel, translation=tr, name=nm)
        assert np.array_equal(r.read_volume(0), want_small) and np.array_equal(r.read_volume(1), fixture)
        same_frame(frame_copy(r.render(frame_64(cam), 0, 2)), want, "grown past its slot")
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_set_volume_restarts_the_reuse_chains(built):
    """reuse_grids_persist: after set_volume the next call looks into no grids of the old medium, as after an upload."""
    flags, options = ["neereservoirs", "neereservoirreuse"], {"reuse_grids_persist": 1}
    fixture, want_small = vc.fixture()["grid"], small_grid()
    sc, cam = scenes.cornell_box(fog=fixture)
    small_sc, _ = scenes.cornell_box(fog=want_small)
    args = dict(ARGS, reservoirM=2, reservoirSpatialM=2, hashGridBucketCount=20000)
    def make():
        r = make_renderer(flags, args)
        r.set_option("reuse_grids_persist", 1)
        return r
    a, b = make(), make()
    try:
        b.update(small_sc)
        want = frame_copy(b.render(frame_64(cam), 1, 1))
        a.update(sc)
        a.render(frame_64(cam), 0, 1)  # (leaves its grids behind)
        a.set_volume(0, grid=want_small)
        same_frame(frame_copy(a.render(frame_64(cam), 1, 1)), want, "the chain restarts")
    finally:
        a.close()
        b.close()
