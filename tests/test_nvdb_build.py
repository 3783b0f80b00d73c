"""The numpy statement of the volume-build contract (stratum_amd/nvdb.py: dense_to_nanovdb; include/sthip.h:
sthip_build_volume) against independent readers, without a GPU: the fixture tests/golden/fog_sphere.npz, which the reference's
vendored NanoVDB wrote, and the oracle's reader (oracle_py.nvdb_probe)."""
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


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle_py

    oracle_py.build()
    return oracle_py


def views(b):
    """The parts of a grid's bytes as structured arrays (the dtypes of nvdb.py, applied at the offsets the tree names)."""
    b = np.ascontiguousarray(b, np.uint8)
    tree = b[672:736].view(nvdb.TREE)[0]
    off = [672 + int(x) for x in tree["node_offset"]]  # leaf, lower, upper, root
    n_leaf, n_low, n_up = (int(x) for x in tree["node_count"])
    root = b[off[3] : off[3] + 64].view(nvdb.ROOT)[0]
    tiles = b[off[3] + 64 : off[3] + 64 + 32 * int(root["table_size"])].view(nvdb.TILE)
    return {
        "grid": b[:672].view(nvdb.GRID)[0], "tree": tree, "root": root, "tiles": tiles,
        "upper": b[off[2] : off[2] + nvdb.UPPER_BYTES * n_up].view(nvdb.UPPER),
        "lower": b[off[1] : off[1] + nvdb.LOWER_BYTES * n_low].view(nvdb.LOWER),
        "leaf": b[off[0] : off[0] + nvdb.LEAF_BYTES * n_leaf].view(nvdb.LEAF),
    }


def test_fixture_rebuilt(oracle):
    """The fixture read through the oracle over its box +- 4 voxels, built again, and compared with the fixture field by field.
    Expected differences, tolerated here and nowhere else: checksum, flags, average / deviation fields, background, name."""
    g = vc.fixture()
    fx = g["grid"]
    dense = vc.fixture_dense()
    coords = vc.box_coords(vc.FIXTURE_ORIGIN, dense.shape)
    # the fixture itself: its active voxels are exactly its non-zero voxels, their box is the root box, the rest reads 0
    f = views(fx)
    lattice = np.zeros((48, 48, 48), bool)  # the leaves' own lattice and the box, index -16 .. 31
    for leaf in f["leaf"]:
        bits = np.unpackbits(leaf["value_mask"], bitorder="little").reshape(8, 8, 8).astype(bool)
        o = (leaf["bbox_min"] & ~7) + 16
        lattice[o[0] : o[0] + 8, o[1] : o[1] + 8, o[2] : o[2] + 8] = bits
    w = np.asarray(vc.FIXTURE_ORIGIN) + 16
    active = lattice[w[0] : w[0] + 28, w[1] : w[1] + 28, w[2] : w[2] + 28]
    assert int(lattice.sum()) == int(active.sum()) == 4192 == int(f["tree"]["voxel_count"])
    assert np.array_equal(active, dense != 0)
    nz = coords[(dense != 0).reshape(-1)]
    assert np.array_equal(nz.min(axis=0), [-8, -10, -7]) and np.array_equal(nz.max(axis=0), [11, 9, 12])
    assert np.array_equal(f["root"]["bbox"], [-8, -10, -7, 11, 9, 12])
    assert (dense[~active] == 0).all()

    built = vc.numpy_grid("fixture")
    assert built.size == fx.size
    b = views(built)
    assert np.array_equal(b["tree"]["node_offset"], f["tree"]["node_offset"])
    assert list(b["tree"]["node_count"]) == [26, 8, 8] == list(f["tree"]["node_count"]) and int(b["root"]["table_size"]) == 8 == int(f["root"]["table_size"])
    assert int(b["tree"]["voxel_count"]) == 4192
    assert np.array_equal(b["tiles"]["key"], f["tiles"]["key"]) and np.array_equal(b["tiles"]["child"], f["tiles"]["child"])
    assert np.array_equal(b["tiles"].view(np.uint8), f["tiles"].view(np.uint8))
    for level in ("upper", "lower"):
        for field in ("bbox", "flags", "child_mask", "value_mask", "table", "min", "max", "pad"):
            assert np.array_equal(b[level][field], f[level][field]), (level, field)
    for field in ("bbox_min", "bbox_dif", "flags", "value_mask", "values", "min", "max"):
        assert np.array_equal(np.ascontiguousarray(b["leaf"][field]).view(np.uint8), np.ascontiguousarray(f["leaf"][field]).view(np.uint8)), field
    assert np.array_equal(b["root"]["bbox"], [-8, -10, -7, 11, 9, 12])
    assert b["root"]["max"] == F32(1.0) == f["root"]["max"] and b["root"]["min"] == f["root"]["min"]
    assert np.array_equal(b["grid"]["world_bbox"], f["grid"]["world_bbox"]) and np.array_equal(b["grid"]["voxel_size"], f["grid"]["voxel_size"])
    for field in ("magic", "version", "grid_index", "grid_count", "grid_size", "matf", "invmatf", "vecf", "taperf", "matd", "invmatd", "vecd", "taperd", "grid_class", "grid_type", "blind_offset", "blind_count"):
        assert np.array_equal(b["grid"][field], f["grid"][field]), field
    # every byte that differs lies in a field of the list above
    allowed = np.zeros(fx.size, bool)
    allowed[8:16] = allowed[20:24] = allowed[40:296] = True  # checksum, flags, name
    r0 = 672 + 64
    allowed[r0 + 28 : r0 + 32] = allowed[r0 + 40 : r0 + 48] = True  # background; average, deviation
    for base, size, n, stat in ((672 + 384, nvdb.UPPER_BYTES, 8, 8232), (672 + int(f["tree"]["node_offset"][1]), nvdb.LOWER_BYTES, 8, 1064), (672 + int(f["tree"]["node_offset"][0]), nvdb.LEAF_BYTES, 26, 88)):
        for i in range(n):
            allowed[base + size * i + stat : base + size * i + stat + 8] = True
    differing = np.flatnonzero(built != fx)
    assert allowed[differing].all(), differing[~allowed[differing]][:10]
    assert int(b["grid"]["checksum"]) == 0xFFFFFFFFFFFFFFFF and int(b["grid"]["flags"]) == 0x26 and int(f["grid"]["flags"]) == 0x3E and b["root"]["background"] == 0
    assert bytes(b["grid"]["name"]) == b"density"

    # the map answers of the fixture, bit for bit, and its probes
    lo, hi, root_max, values, maps = oracle.nvdb_probe(built, g["coords"], g["map"][:, 0])
    assert np.array_equal(lo, g["bbox_min"]) and np.array_equal(hi, g["bbox_max"]) and F32(root_max) == g["root_max"]
    assert np.array_equal(maps.view(np.uint32), g["map"][:, 1:, :].view(np.uint32))  # the four map functions at 16 points
    o, n = np.asarray(vc.FIXTURE_ORIGIN), vc.FIXTURE_N
    inside = ((g["coords"] >= o) & (g["coords"] < o + n)).all(axis=1)
    # Compared with the fixture: every probe under one of its eight root tiles (index -4096 .. 4095), which holds every probe
    # inside the dense box (2 454 of them) and the near ones around it, where the fixture's inactive tiles read 0 as well. Left
    # out: the far probes under no tile, where the fixture reads its root background 0.24, a leftover of the level set it was
    # made from and not this contract. One probe in sixteen is drawn from +-5000, so at least 5 600 remain compared.
    compared = ((g["coords"] >= -4096) & (g["coords"] < 4096)).all(axis=1)
    assert (compared | ~inside).all() and int(inside.sum()) > 2000 and int(compared.sum()) >= 5600
    assert np.array_equal(values[compared].view(np.uint32), g["values"][compared].view(np.uint32))
    assert (values[~inside].view(np.uint32) == 0).all() and (g["values"][~compared] == F32(0.24)).all()


@pytest.mark.parametrize("name", list(vc.CASES))
def test_every_voxel_through_the_oracles_reader(oracle, name):
    """Every voxel of the box reads back as the dense value (-0.0f as +0), a shell of 3 voxels around it and far probes read 0,
    and the header answers are exact."""
    dense, origin, voxel, tr, nm = vc.case(name)
    grid = vc.numpy_grid(name)
    shell = 3
    o = np.asarray(origin) - shell
    shape = tuple(s + 2 * shell for s in dense.shape)
    want = np.zeros(shape, F32)
    want[shell:-shell, shell:-shell, shell:-shell] = np.where(dense != 0, dense, F32(0))
    coords = np.concatenate([vc.box_coords(o, shape), np.array([[5000, -5000, 3], [-(2**31), 2**31 - 1, 0], [origin[0] + 4096, origin[1], origin[2]]], np.int32)])
    lo, hi, root_max, values, _ = oracle.nvdb_probe(grid, coords, np.zeros((1, 3), F32))
    assert np.array_equal(values[: want.size].view(np.uint32), want.reshape(-1).view(np.uint32))
    assert (values[want.size :].view(np.uint32) == 0).all()
    nz = np.argwhere(dense != 0) + np.asarray(origin)
    assert np.array_equal(lo, nz.min(axis=0)) and np.array_equal(hi, nz.max(axis=0))
    active = dense[dense != 0]
    assert F32(root_max) == active.max()
    v = views(grid)
    assert v["root"]["min"] == active.min() and int(v["tree"]["voxel_count"]) == active.size
    info = nvdb.grid_info(grid)
    assert np.array_equal(info["world_bbox"][:3], nz.min(axis=0) * float(voxel) + np.asarray(tr)) and np.array_equal(info["world_bbox"][3:], (nz.max(axis=0) + 1) * float(voxel) + np.asarray(tr))
    # exact boxes and min/max at every level, from the dense array
    for leaf in v["leaf"]:
        c0 = (leaf["bbox_min"].astype(np.int64) >> 3) << 3
        inside = ((nz >= c0) & (nz < c0 + 8)).all(axis=1)
        assert inside.any()
        assert np.array_equal(leaf["bbox_min"], nz[inside].min(axis=0)) and np.array_equal(leaf["bbox_dif"], nz[inside].max(axis=0) - nz[inside].min(axis=0))
        vals = active[inside]
        assert leaf["min"] == vals.min() and leaf["max"] == vals.max() and leaf["flags"] == 2
    for level, shift in (("lower", 7), ("upper", 12)):
        for node in v[level]:
            c0 = (node["bbox"][:3].astype(np.int64) >> shift) << shift
            inside = ((nz >= c0) & (nz < c0 + (1 << shift))).all(axis=1)
            assert np.array_equal(node["bbox"][:3], nz[inside].min(axis=0)) and np.array_equal(node["bbox"][3:], nz[inside].max(axis=0))
            assert node["min"] == active[inside].min() and node["max"] == active[inside].max()
    if name == "cropped":
        assert list(v["tree"]["node_count"][1:]) == [4, 4] and len(v["tiles"]) == 4  # x = 0 and z = 4096 are root-tile boundaries
        keys = [(int(k) >> 42, (int(k) >> 21) & 0x1FFFFF, int(k) & 0x1FFFFF) for k in v["tiles"]["key"]]
        assert keys == [(0xFFFFF, 0, 0), (0xFFFFF, 0, 1), (0, 0, 0), (0, 0, 1)]  # the tiles at x = -1 come first: signed order
    if name == "skip":
        assert list(v["tree"]["node_count"]) == [16 + 6, 2, 1]  # z 0..127 and 256..299: the middle lower node does not exist
    if name == "bricks":
        assert int(v["tree"]["node_count"][0]) == 26  # 27 bricks, the middle one empty; the constant one stays a leaf
        constant = [leaf for leaf in v["leaf"] if (leaf["values"] == F32(0.75)).all()]
        assert len(constant) == 1 and np.array_equal(constant[0]["bbox_min"], [0, 0, 16]) and (constant[0]["value_mask"] == 255).all()
    if name == "signs":
        assert v["root"]["min"] == F32(-1.5) and v["root"]["max"] == F32(2.0) and (dense == 0).any() and np.signbit(dense[dense == 0]).any()


def test_refusals():
    one = np.ones((2, 2, 2), F32)
    for bad, kwargs in (
        (np.array([[[np.nan]]], F32), {}),
        (np.array([[[np.inf, 1.0]]], F32), {}),
        (np.zeros((3, 3, 3), F32), {}),
        (np.full((1, 1, 1), -0.0, F32), {}),
        (one, {"voxel_size": 0.0}),
        (one, {"voxel_size": -1.0}),
        (one, {"voxel_size": np.inf}),
        (one, {"voxel_size": np.nan}),
        (one, {"origin": (2**31 - 1, 0, 0)}),
        (one, {"name": "x" * 256}),
    ):
        with pytest.raises(ValueError):
            nvdb.dense_to_nanovdb(bad, **kwargs)
    nvdb.dense_to_nanovdb(one, origin=(2**31 - 2, -(2**31), 0))  # the last coordinates int32 holds


def test_scene_builder_dense_volume_renders_as_the_same_bytes(oracle):
    """SceneBuilder.add_dense_volume is add_volume of the numpy statement's bytes: the same scene arrays and, through the
    oracle, the same frame as the fixture's grid gives (the rebuilt grid answers every lookup inside the box alike)."""
    from stratum_amd.scene import SceneBuilder

    dense, origin, voxel, tr, nm = vc.case("fixture")
    a, b = SceneBuilder("a"), SceneBuilder("b")
    for s, vol in ((a, a.add_dense_volume(dense, origin, voxel, tr, nm)), (b, b.add_volume(vc.numpy_grid("fixture")))):
        quad = s.add_mesh(*scenes._quad((-1, -1, -1), (1, -1, -1), (1, -1, 1), (-1, -1, 1), (0, 1, 0)))
        s.add_instance(quad, s.add_emitter((5.0, 5.0, 5.0)))
        s.add_medium(vol, density_scale=(3, 3, 3), albedo_scale=(0.9, 0.9, 0.9))
    sa, sb = a.build(), b.build()
    assert len(sa.volumes) == 1 and np.array_equal(sa.volumes[0], sb.volumes[0]) and np.array_equal(sa.instances, sb.instances)
    cam = scenes.cornell_box()[1]
    frame = camera.Frame(24, 16, cam["fovy"], cam["eye"], cam["target"])
    pc = wire.default_push_constants(24, 16, sa.light_count)
    ra = oracle.OracleScene(sa).render(frame, pc, wire.DEFAULT_SAMPLING_FLAGS, 0, 1)
    fog_sc = scenes.cornell_box(fog=vc.numpy_grid("fixture"))[0]
    fix_sc = scenes.cornell_box(fog=vc.fixture()["grid"])[0]
    pc = wire.default_push_constants(24, 16, fog_sc.light_count)
    rb = oracle.OracleScene(fog_sc).render(frame, pc, wire.DEFAULT_SAMPLING_FLAGS, 0, 1)
    rf = oracle.OracleScene(fix_sc).render(frame, pc, wire.DEFAULT_SAMPLING_FLAGS, 0, 1)
    assert np.isfinite(ra["radiance"]).all()
    assert np.array_equal(rb["radiance"].view(np.uint32), rf["radiance"].view(np.uint32)) and np.array_equal(rb["ray_count"], rf["ray_count"])
    assert (rb["radiance"][..., :3] > 0).any()


def test_the_uploads_host_checks_accept_the_bytes(tmp_path):
    """check_scene of the upload (csrc/scene_prepare.cpp), as a CPU program, accepts a scene whose grid the numpy statement made."""
    import test_host_cpp as h

    exe = str(tmp_path / "scene_prepare_check")
    csrc = os.path.join(ROOT, "stratum_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "cpp", "scene_prepare_check.cpp"), os.path.join(csrc, "scene_prepare.cpp"),
                           os.path.join(csrc, "bvh_build.cpp"), "-lpthread"])
    sc = scenes.cornell_box(fog=vc.numpy_grid("cropped"))[0]
    assert h._run_prepare(exe, "check", h._dump_arrays(tmp_path / "scene", sc)) == "ACCEPTED\n"
    # ... and the header checks of the tree build (bvh_build.cpp:344-378), restated on the bytes
    g = vc.numpy_grid("cropped")
    assert g.size >= 672 + 64 + 64 and g.size % 4 == 0 and int(g[:8].view("<u8")[0]) == 0x304244566F6E614E and int(g[636:640].view("<u4")[0]) == 1
    root = 672 + int(g[672 + 24 : 672 + 32].view("<u8")[0])
    tiles = int(g[root + 24 : root + 28].view("<u4")[0])
    assert root + 64 + 32 * tiles <= g.size and tiles <= 65536


def test_layout_order_equals_a_sort(tmp_path):
    """csrc/volume_build.h: the closed-form slot of a brick and of a lower cell is its rank under the breadth-first key, and a
    cell's children are consecutive slots (tests/cpp/volume_slots_check.cpp, under ASan + UBSan)."""
    exe = str(tmp_path / "volume_slots_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "cpp", "volume_slots_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr[-2000:]
