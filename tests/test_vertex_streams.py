"""Vertices from device memory: sthip_scene_set_vertices packs strided position / normal / uv streams into the resident
gVertices (k_pack_vertices, stratum_amd/csrc/vertex_streams.hip) and makes the shading normals of the written range again from
the moved positions (k_face_vectors, k_vertex_normals); the gather and the refit of sthip_scene_update_vertices follow. Both
contracts are part of the header (include/sthip.h): the pack is bit copies, the normals are binary32, unfused, summed in
ascending (mesh, triangle, corner). `packed` and `recomputed` below restate them with numpy's float32 operations, which are
correctly rounded and unfused, so every comparison here is of bits, without a tolerance."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from stratum_amd import camera, scenes, wire
from stratum_amd.scene import rotate_x, rotate_y, scale, translate

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_refit import deformed, make_renderer, same_frame  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SRC = os.path.join(ROOT, "tests", "cpp", "vertex_streams_check.cpp")
HOST_SRC = os.path.join(ROOT, "tests", "cpp", "vertex_streams_host.cpp")
CXX = os.environ.get("CXX", "g++")
f32 = np.float32


def bits(v):
    return np.ascontiguousarray(v).view(np.uint32)


def rows(v):
    """The records as (n, 8) words."""
    return bits(v).reshape(-1, 8)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference: both contracts of include/sthip.h in numpy float32
# ---------------------------------------------------------------------------------------------------------------------------
def packed(resident, first, positions, normals=None, texcoords=None):
    """The pack contract: record first + i becomes {positions[i], u, normals[i], v}, bit copies; an absent stream keeps the
    resident bits; records outside the range are not written."""
    out = resident.copy()
    n = positions.shape[0]
    part = out[first : first + n]
    part["position"] = positions
    if normals is not None:
        part["normal"] = normals
    if texcoords is not None:
        part["u"], part["v"] = texcoords[:, 0], texcoords[:, 1]
    return out


def meshes_of(sc):
    """The meshes of the normal contract: the distinct tuples (indices_byte_offset, first_vertex, index_stride, prim_count) of
    the triangle instances, ascending."""
    out = set()
    for p in sc.instances["packed"]:
        if int(p[0]) & 0xF == wire.INSTANCE_TYPE_TRIANGLES:
            out.add((int(p[3]), int(p[2]), int(p[1]) >> 28, (int(p[1]) >> 12) & 0xFFFF))
    return sorted(out)


def triangles_of(sc):
    """Per mesh, in the contract's order, its absolute index triples (prims, 3)."""
    out = []
    for offset, first, stride, prims in meshes_of(sc):
        raw = np.frombuffer(sc.indices[offset : offset + 3 * prims * stride].tobytes(), dtype="<u2" if stride == 2 else "<u4")
        out.append(raw.astype(np.int64).reshape(prims, 3) + first)
    return out


def recomputed(records, triangles, first, count):
    """The normal contract over records [first, first + count): `records` hold the positions after the call's write. A Python
    loop over the corners in ascending (mesh, triangle, corner); every operation is one float32 operation."""
    out = records.copy()
    pos = records["position"]
    assert pos.dtype == np.float32
    s = np.zeros((records.shape[0], 3), dtype=np.float32)
    with np.errstate(all="ignore"):
        for tris in triangles:
            for t in tris:
                p0, p1, p2 = pos[t[0]], pos[t[1]], pos[t[2]]
                e1, e2 = p1 - p0, p2 - p0
                g = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], dtype=np.float32)
                assert e1.dtype == np.float32 and (e1[1] * e2[2]).dtype == np.float32
                for c in range(3):
                    s[t[c]] = s[t[c]] + g
        d = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
        assert d.dtype == np.float32
        inv = f32(1) / np.sqrt(d)
        unit = s * inv[:, None]
    take = (d > 0) & (d < np.inf)
    take[:first] = False
    take[first + count :] = False
    normal = out["normal"]
    normal[take] = unit[take]
    out["normal"] = normal
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_library_exports_set_vertices(built):
    from stratum_amd import _lib

    assert "sthip_scene_set_vertices" in _lib.EXPORTS and hasattr(_lib.lib(), "sthip_scene_set_vertices")
    assert _lib.lib().sthip_abi_version() == 11


def test_header_declares_set_vertices_and_both_contracts():
    raw = open(os.path.join(ROOT, "include", "sthip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"int\s+sthip_scene_set_vertices\s*\(\s*sthip_ctx\s*\*\s*\w*\s*,\s*const\s+sthip_vertex_streams\s*\*\s*\w*\s*,\s*sthip_refit_info\s*\*\s*\w*\s*\)", text)
    assert "typedef struct sthip_vertex_streams" in text
    assert re.search(r"#define\s+STHIP_ABI_VERSION\s+11\b", text)
    assert "PACK CONTRACT" in raw and "NORMAL CONTRACT" in raw
    host = open(os.path.join(ROOT, "stratum_amd", "host", "stratum_hip.hpp")).read()
    assert re.search(r"#pragma\s+weak\s+sthip_scene_set_vertices\b", host) and "set_vertices_device" in host


def test_mirror_has_the_layout_of_the_c_struct(built, tmp_path):
    fields = [f for f, _ in wire.VertexStreams._fields_]
    assert fields == ["struct_size", "first_vertex", "vertex_count", "device_ptr", "recompute_normals", "position_stride", "normal_stride", "texcoord_stride", "positions", "normals", "texcoords"]
    src = tmp_path / "layout.c"
    prints = "".join('  printf("%%zu\\n", offsetof(sthip_vertex_streams, %s));\n' % f for f in fields)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sthip.h"\nint main(void) {\n  printf("%zu\\n", sizeof(sthip_vertex_streams));\n' + prints + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert got[0] == C.sizeof(wire.VertexStreams) == wire.VERTEX_STREAMS_BYTES
    assert got[1:] == [getattr(wire.VertexStreams, f).offset for f in fields]


def _records(positions, normal=(0.5, 0.25, 0.125)):
    v = np.zeros(len(positions), dtype=wire.PackedVertexData)
    v["position"], v["normal"], v["u"], v["v"] = np.asarray(positions, np.float32), normal, 0.25, 0.75
    return v


def test_the_numpy_statement_on_values_worked_by_hand():
    """The reference itself, on numbers that are exact in binary32."""
    kept = [0.5, 0.25, 0.125]  # (not a unit vector: a normal that stays is a bit copy, not a renormalisation)
    # one triangle in the xy plane: (1,0,0) x (0,1,0) = (0,0,1) at all three vertices
    v = _records([(0, 0, 0), (1, 0, 0), (0, 1, 0)])
    got = recomputed(v, [np.array([[0, 1, 2]])], 0, 3)
    assert got["normal"].tolist() == [[0, 0, 1]] * 3
    assert np.array_equal(bits(got["position"]), bits(v["position"])) and got["u"].tolist() == [0.25] * 3 and got["v"].tolist() == [0.75] * 3
    # two coplanar faces of different area at vertex 0: g = (0,0,1) and (0,0,4), s = (0,0,5), d = 25, 5 * (1 / 5) rounds to 1
    v = _records([(0, 0, 0), (1, 0, 0), (0, 1, 0), (-2, 0, 0), (0, -2, 0)])
    got = recomputed(v, [np.array([[0, 1, 2], [0, 3, 4]])], 0, 5)
    assert got["normal"][0].tolist() == [0, 0, 1] and f32(5) * (f32(1) / f32(5)) == f32(1)
    assert got["normal"][1].tolist() == [0, 0, 1] and got["normal"][3].tolist() == [0, 0, 1]
    # ... and two faces at right angles: the larger one weighs more. g = (0,0,3) and (4,0,0): s = (4,0,3), d = 25
    v = _records([(0, 0, 0), (1, 0, 0), (0, 3, 0), (0, 2, 0), (0, 0, 2)])
    got = recomputed(v, [np.array([[0, 1, 2]]), np.array([[0, 3, 4]])], 0, 5)
    fifth = f32(1) / f32(5)
    assert got["normal"][0].tolist() == [f32(4) * fifth, 0, f32(3) * fifth]
    assert got["normal"][1].tolist() == [0, 0, 1] and got["normal"][3].tolist() == [1, 0, 0]
    # only the range is written: outside it the normals stay, and the positions there still contribute
    part = recomputed(v, [np.array([[0, 1, 2]]), np.array([[0, 3, 4]])], 0, 1)
    assert part["normal"][0].tolist() == got["normal"][0].tolist() and part["normal"][1:].tolist() == [kept] * 4
    # a vertex of two opposite faces keeps its normal: (0,0,1) + (0,0,-1) = 0 at all three vertices
    v = _records([(0, 0, 0), (1, 0, 0), (0, 1, 0)])
    got = recomputed(v, [np.array([[0, 1, 2], [0, 2, 1]])], 0, 3)
    assert np.array_equal(rows(got), rows(v))
    # a vertex no triangle names keeps its normal, and so does one whose only face is degenerate (a repeated index)
    v = _records([(0, 0, 0), (1, 0, 0), (0, 1, 0), (5, 5, 5), (7, 7, 7)])
    got = recomputed(v, [np.array([[0, 1, 2], [1, 4, 4]])], 0, 5)
    assert got["normal"][3].tolist() == kept and got["normal"][4].tolist() == kept and got["normal"][1].tolist() == [0, 0, 1]
    # a NaN in the sum: the normal stays
    v = _records([(0, 0, 0), (1, 0, 0), (0, np.nan, 0)])
    got = recomputed(v, [np.array([[0, 1, 2]])], 0, 3)
    assert got["normal"].tolist() == [kept] * 3
    # the pack: bit copies, absent streams stay, records outside the range stay
    v = _records([(0, 0, 0), (1, 0, 0), (0, 1, 0), (2, 2, 2)])
    p = np.array([[9, 8, 7], [-0.0, 6, 5]], dtype=np.float32)
    got = packed(v, 1, p)
    assert np.array_equal(rows(got)[[0, 3]], rows(v)[[0, 3]]) and np.array_equal(bits(got["position"][1:3]), bits(p))
    assert np.array_equal(bits(got["normal"]), bits(v["normal"])) and got["u"].tolist() == [0.25] * 4
    got = packed(v, 1, p, normals=p[::-1], texcoords=p[:, :2])
    assert np.array_equal(bits(got["normal"][1:3]), bits(p[::-1])) and np.array_equal(bits(got["u"][1:3]), bits(p[:, 0])) and np.array_equal(bits(got["v"][1:3]), bits(p[:, 1]))


def test_refusals_and_the_mesh_list_on_the_host_under_sanitizers(tmp_path):
    """tests/cpp/vertex_streams_check.cpp links scene_prepare.cpp only: every refusal of the header returns its code and names
    the field, every accepted description passes, the mesh list comes out in the contract's order — under
    -fsanitize=address,undefined."""
    exe = str(tmp_path / "vertex_streams_check")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-o", exe, CHECK_SRC,
                           os.path.join(ROOT, "stratum_amd", "csrc", "scene_prepare.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "VERTEX STREAMS CHECK OK" in out.stdout and "FAIL" not in out.stdout, out.stdout + out.stderr
    for case in ("no scene", "struct_size", "NULL positions", "range past vertex_count", "positions unaligned", "normals unaligned", "texcoords unaligned",
                 "position_stride not a multiple of 4", "normal_stride not a multiple of 4", "texcoord_stride not a multiple of 4", "position_stride below 12",
                 "normal_stride below 12", "texcoord_stride below 8", "normals with recompute_normals", "empty range", "order, shared tuples, strides, aligned offset"):
        assert re.search(r"^ok\s+%s" % re.escape(case), out.stdout, re.M), case


# ---------------------------------------------------------------------------------------------------------------------------
# the scene: the Cornell box with three meshes appended
# ---------------------------------------------------------------------------------------------------------------------------
GRID_W, GRID_H, FAN = 5, 4, 70


def streams_scene():
    """(scene, camera, names): the Cornell box, then a 5 x 4 vertex grid with 16-bit indices under two transformed instances
    (a shared mesh), then a fan with 32-bit indices under an identity instance (it lies in the merged mesh): a hub of valence 70
    (more than a wave), one degenerate triangle (a repeated index) that is the only face of one vertex, and three records no
    index names. `names`: the record numbers the tests check by name."""
    sc, cam = scenes.cornell_box()
    b = sc.builder
    own = sc.vertices.shape[0]
    white = 0
    pos = np.array([(0.12 * x, 0.03 * ((x * y) % 3), 0.12 * y) for y in range(GRID_H) for x in range(GRID_W)], dtype=np.float32)
    uv = np.array([(x / (GRID_W - 1), y / (GRID_H - 1)) for y in range(GRID_H) for x in range(GRID_W)], dtype=np.float32)
    tri = []
    for y in range(GRID_H - 1):
        for x in range(GRID_W - 1):
            a = y * GRID_W + x
            tri += [(a, a + GRID_W, a + 1), (a + 1, a + GRID_W, a + GRID_W + 1)]
    grid = b.add_mesh(pos, np.tile(np.array([0, 1, 0], np.float32), (pos.shape[0], 1)), uv, tri, index_stride=2)
    b.add_instance(grid, white, translate((-0.75, -0.55, 0.35)) @ rotate_y(0.3))
    b.add_instance(grid, white, translate((0.2, -0.2, 0.2)) @ rotate_x(0.5) @ scale((0.8, 0.8, 0.8)))
    angle = 2 * np.pi * np.arange(FAN) / FAN
    rim = np.stack([0.28 * np.cos(angle), 0.02 * np.sin(3 * angle), 0.28 * np.sin(angle)], axis=1)
    centre = np.array([-0.15, -0.8, 0.6])
    lone = np.array([[0.3, 0.0, 0.3]])  # named by the degenerate triangle only
    spare = np.array([[0.5, 0.1, 0.1], [0.5, 0.2, 0.1], [0.5, 0.3, 0.1]])  # named by no index
    fpos = (np.concatenate([[[0, 0.12, 0]], rim, lone, spare]) + centre).astype(np.float32)
    rng = np.random.default_rng(11)
    fnrm = rng.standard_normal((fpos.shape[0], 3))
    fnrm = (fnrm / np.linalg.norm(fnrm, axis=1, keepdims=True)).astype(np.float32)
    ftri = [(0, 1 + (i + 1) % FAN, 1 + i) for i in range(FAN)] + [(1, FAN + 1, FAN + 1)]
    fan = b.add_mesh(fpos, fnrm, rng.random((fpos.shape[0], 2)).astype(np.float32), ftri, index_stride=4)
    b.add_instance(fan, white)
    out = b.build()
    grid_first, fan_first = own, own + GRID_W * GRID_H
    names = {
        "own": own,
        "grid": (grid_first, GRID_W * GRID_H),
        "grid_instances": (out.instances.shape[0] - 3, out.instances.shape[0] - 2),
        "fan_instance": out.instances.shape[0] - 1,
        "hub": fan_first,
        "lone": fan_first + 1 + FAN,
        "spare": [fan_first + 2 + FAN + k for k in range(3)],
        "degenerate_corner": fan_first + 1,  # a rim vertex the degenerate triangle names too
    }
    assert out.vertices.shape[0] == fan_first + FAN + 5 == 139 and out.triangle_count == 32 + 2 * 24 + FAN + 1
    return out, cam, names


def frame_of(cam):
    return camera.Frame(64, 64, cam["fovy"], cam["eye"], cam["target"])


def render(r, cam):
    return r.render(frame_of(cam), 0, 1)


def on_device(*arrays):
    import torch

    out = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]
    torch.cuda.synchronize()
    return out


def new_streams(sc, first, count, seed):
    """(positions, normals, texcoords) for records [first, first + count): positions near the resident ones (the tree stays
    sane), normals and uvs with bit patterns only a bit copy keeps (-0, a denormal, a NaN with a payload)."""
    rng = np.random.default_rng(seed)
    p = (sc.vertices["position"][first : first + count] + rng.uniform(-0.02, 0.02, (count, 3))).astype(np.float32)
    n = rng.standard_normal((count, 3)).astype(np.float32)
    t = rng.random((count, 2)).astype(np.float32)
    special = np.array([0x80000000, 0x00000001, 0x7FC12345, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)
    n.reshape(-1)[: min(4, n.size)] = special[: min(4, n.size)]
    t.reshape(-1)[: min(2, t.size)] = special[2 : 2 + min(2, t.size)]
    return p, n, t


def wrong_rows(got, expected):
    return np.flatnonzero((rows(got) != rows(expected)).any(axis=1))


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: records
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pack_from_device_streams_is_bit_copies_and_leaves_the_rest(built):
    """Case 1: tight torch tensors; ranges from record 1 with 1, 63, 64 and 65 records, then the whole scene."""
    sc, _, _ = streams_scene()
    n = sc.vertices.shape[0]
    r = make_renderer()
    try:
        r.update(sc)
        expected = sc.vertices.copy()
        assert np.array_equal(rows(r.read_vertices(0, n)), rows(expected))
        for k, (first, count) in enumerate([(1, 1), (1, 63), (1, 64), (1, 65), (0, n)]):
            p, nrm, uv = new_streams(sc, first, count, 20 + k)
            dp, dn, dt = on_device(p, nrm, uv)
            assert dp.stride(0) == 3 and dt.stride(0) == 2
            info = r.set_vertices(first, dp, dn, dt)
            assert info["rebuilt"] == 0 and info["device_ms"] > 0
            before = expected
            expected = packed(expected, first, p, nrm, uv)
            got = r.read_vertices(0, n)
            wrong = wrong_rows(got, expected)
            assert wrong.size == 0, (first, count, wrong[:8], got[wrong[:2]], expected[wrong[:2]])
            outside = np.r_[0:first, first + count : n]
            assert np.array_equal(rows(got)[outside], rows(before)[outside])
            assert (rows(got)[first : first + count] != rows(before)[first : first + count]).any(axis=1).all()  # (every record of the range changed)
    finally:
        r.close()


@pytest.mark.gpu
def test_strides_alignment_and_the_host_form(built):
    """Case 2: one interleaved 32-byte-stride buffer, a stride of 20, a base that is 4- but not 8-byte aligned, a torch view with
    a row stride; the host form with numpy views of the same layouts gives the same records."""
    import torch

    sc, _, _ = streams_scene()
    n = sc.vertices.shape[0]
    first, count = 3, 101
    p, nrm, uv = new_streams(sc, first, count, 31)
    want = packed(sc.vertices, first, p, nrm, uv)

    def layouts(xp_zeros, place):
        inter = xp_zeros((count, 8))  # [position | normal | uv]: 32 bytes per vertex
        place(inter[:, 0:3], p), place(inter[:, 3:6], nrm), place(inter[:, 6:8], uv)
        wide = xp_zeros((count, 5))  # a stride of 20 bytes
        place(wide[:, 0:3], p)
        flat = xp_zeros(1 + 3 * count)  # the stream starts 4 bytes into an allocation
        odd = flat[1:].reshape(count, 3)
        place(odd, nrm)
        skip = xp_zeros((2 * count, 2))  # every other row: a row stride of 16 bytes
        place(skip[::2], uv)
        return inter, wide, odd, skip[::2]

    def place_torch(dst, src):
        dst.copy_(torch.from_numpy(src))

    def place_numpy(dst, src):
        dst[...] = src

    r = make_renderer()
    try:
        for form in ("device", "host"):
            r.update(sc)
            if form == "device":
                inter, wide, odd, skip = layouts(lambda shape: torch.zeros(shape, dtype=torch.float32, device="cuda:0"), place_torch)
                torch.cuda.synchronize()
                assert odd.data_ptr() % 8 == 4 and wide.stride(0) == 5 and skip.stride(0) == 4 and inter.stride(0) == 8
            else:
                inter, wide, odd, skip = layouts(lambda shape: np.zeros(shape, np.float32), place_numpy)
                assert odd.ctypes.data % 8 == 4 and wide.strides[0] == 20 and skip.strides[0] == 16 and inter.strides[0] == 32
            r.set_vertices(first, inter[:, 0:3], inter[:, 3:6], inter[:, 6:8])
            wrong = wrong_rows(r.read_vertices(0, n), want)
            assert wrong.size == 0, (form, "interleaved", wrong[:8])
            r.update(sc)
            r.set_vertices(first, wide[:, 0:3], odd, skip)
            wrong = wrong_rows(r.read_vertices(0, n), want)
            assert wrong.size == 0, (form, "strided", wrong[:8])
    finally:
        r.close()


@pytest.mark.gpu
def test_absent_streams_keep_the_resident_fields(built):
    """Case 3: texcoords = None keeps u and v, normals = None without recompute keeps the normals."""
    sc, _, _ = streams_scene()
    n = sc.vertices.shape[0]
    first, count = 5, 67
    p, nrm, uv = new_streams(sc, first, count, 41)
    r = make_renderer()
    try:
        for streams in ((p, None, None), (p, nrm, None), (p, None, uv)):
            r.update(sc)
            r.set_vertices(first, *on_device(*streams))
            want = packed(sc.vertices, first, *streams)
            wrong = wrong_rows(r.read_vertices(0, n), want)
            assert wrong.size == 0, ([s is not None for s in streams], wrong[:8])
            if streams[1] is None:
                assert np.array_equal(bits(want["normal"]), bits(sc.vertices["normal"]))
            if streams[2] is None:
                assert np.array_equal(bits(want["u"]), bits(sc.vertices["u"])) and np.array_equal(bits(want["v"]), bits(sc.vertices["v"]))
    finally:
        r.close()


@pytest.mark.gpu
def test_recomputed_normals_equal_the_numpy_statement(built):
    """Case 4: the whole scene, then a sub-range that cuts through the grid; the hub, the degenerate cases, the unreferenced
    records and the shared mesh by name; a second call with the same positions gives the same bytes."""
    sc, _, names = streams_scene()
    n = sc.vertices.shape[0]
    triangles = triangles_of(sc)
    grid_first, grid_count = names["grid"]
    assert sum(1 for m in meshes_of(sc) if m[1] == grid_first) == 1  # two instances, one mesh: its corners count once
    assert len(meshes_of(sc)) == sc.instances.shape[0] - 2 == 9  # (the Cornell box's two blocks share a mesh as well)
    moved = deformed(sc.vertices, 0.05)["position"]
    r = make_renderer()
    try:
        r.update(sc)
        (dp,) = on_device(moved)
        info = r.set_vertices(0, dp, recompute_normals=True)
        assert info["rebuilt"] == 0 and info["device_ms"] > 0
        want = recomputed(packed(sc.vertices, 0, moved), triangles, 0, n)
        got = r.read_vertices(0, n)
        wrong = wrong_rows(got, want)
        assert wrong.size == 0, (wrong[:8], got[wrong[:2]], want[wrong[:2]])
        kept = lambda v: np.array_equal(bits(got["normal"][v]), bits(sc.vertices["normal"][v]))  # noqa: E731
        hub = names["hub"]
        assert sum(int((t == hub).sum()) for t in triangles) == FAN > 64 and not kept(hub)
        assert abs(float(np.linalg.norm(got["normal"][hub].astype(np.float64))) - 1) < 1e-6
        assert kept(names["lone"]) and all(kept(v) for v in names["spare"])  # only degenerate faces; no face at all
        assert not kept(names["degenerate_corner"])  # its degenerate face adds +0 to the faces of the fan
        assert not any(kept(v) for v in range(grid_first, grid_first + grid_count))
        assert np.array_equal(bits(got["u"]), bits(sc.vertices["u"])) and np.array_equal(bits(got["v"]), bits(sc.vertices["v"]))
        r.set_vertices(0, dp, recompute_normals=True)
        assert np.array_equal(rows(r.read_vertices(0, n)), rows(got)), "the same positions, other bytes"
        # a sub-range that cuts through the grid: neighbours outside contribute their positions and keep their normals
        first, count = grid_first + 7, 9
        again = deformed(want[first : first + count], 0.04, freq=5.0, phase=0.7)["position"]
        (dq,) = on_device(again)
        r.set_vertices(first, dq, recompute_normals=True)
        want2 = recomputed(packed(want, first, again), triangles, first, count)
        got2 = r.read_vertices(0, n)
        wrong = wrong_rows(got2, want2)
        assert wrong.size == 0, (wrong[:8], got2[wrong[:2]], want2[wrong[:2]])
        outside = np.r_[0:first, first + count : n]
        assert np.array_equal(rows(got2)[outside], rows(got)[outside])
        whole = recomputed(packed(want, first, again), triangles, 0, n)
        assert (bits(whole["normal"])[outside] != bits(want2["normal"])[outside]).any()  # (the neighbours would have changed)
        # the host form gives the same records
        r.update(sc)
        r.set_vertices(0, moved, recompute_normals=True)
        assert np.array_equal(rows(r.read_vertices(0, n)), rows(want))
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: frames
# ---------------------------------------------------------------------------------------------------------------------------
def deformed_scene():
    """(scene as uploaded, camera, names, moved positions, the scene with the statement's records)"""
    sc, cam, names = streams_scene()
    moved = deformed(sc.vertices, 0.05)["position"]
    ref, _, _ = streams_scene()
    ref.vertices[:] = recomputed(packed(sc.vertices, 0, moved), triangles_of(sc), 0, sc.vertices.shape[0])
    return sc, cam, names, moved, ref


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [1, 0])
@pytest.mark.parametrize("wide", [0, 1, 3])
@pytest.mark.parametrize("builder", [0, 1])
def test_frames_equal_the_host_path_and_a_fresh_upload(built, builder, wide, keep):
    """Case 5: a sine displacement. The frame after set_vertices from device streams with recomputed normals, the frame after
    update_vertices with the statement's records on the same context and the frame of a fresh upload of those records are equal
    word for word. wide_bvh = 3 over a host-built tree is the 8-wide form, which is built again from the kept scene
    (rebuilt = 1; a device-built tree has the 4-wide form under that option and is refitted); without a kept scene that
    layout returns unsupported and the records and the frame are unchanged."""
    from stratum_amd._lib import StratumHipError

    sc, cam, _, moved, ref = deformed_scene()
    n = sc.vertices.shape[0]
    rebuilds_again = wide == 3 and builder == 0
    r = make_renderer(options={"bvh_builder": builder, "wide_bvh": wide, "keep_scene": keep})
    try:
        r.update(sc)
        before = render(r, cam)
        (dp,) = on_device(moved)
        if rebuilds_again and not keep:
            with pytest.raises(StratumHipError) as e:
                r.set_vertices(0, dp, recompute_normals=True)
            assert "(-4)" in str(e.value) and "keep_scene" in str(e.value)  # STHIP_ERR_UNSUPPORTED
            assert np.array_equal(rows(r.read_vertices(0, n)), rows(sc.vertices))
            same_frame(render(r, cam), before, "refused: the old scene")
            return
        info = r.set_vertices(0, dp, recompute_normals=True)
        assert info["rebuilt"] == (1 if rebuilds_again else 0), info
        assert np.array_equal(rows(r.read_vertices(0, n)), rows(ref.vertices))
        got = render(r, cam)
        assert not np.array_equal(before["radiance"], got["radiance"])
        r.update(sc)  # (the undeformed scene again, so that the host call has something to change)
        plain, _, _ = streams_scene()
        plain.set_vertices(0, ref.vertices)
        r.update_vertices(plain)
        same_frame(got, render(r, cam), "(a) the statement's records through update_vertices")
        r.update(ref)
        same_frame(got, render(r, cam), "(b) a fresh upload of the statement's records")
    finally:
        r.close()


@pytest.mark.gpu
def test_the_kept_scene_follows_before_anything_is_built_from_it(built):
    """Case 6: after set_vertices from device streams the kept scene is behind. Moving the identity instance of the fan forces
    a rebuild from it: the frame is that of a fresh upload of the new vertices and the new transforms. A host update_vertices
    over an overlapping sub-range in between makes that part current: the frame is that of the combined records."""
    sc, cam, names, moved, ref = deformed_scene()
    n = sc.vertices.shape[0]
    fan = names["fan_instance"]
    assert np.array_equal(sc.transforms["m"][fan], np.eye(4, dtype=np.float32)[:3])
    shift = translate((0.05, 0.1, -0.1)) @ rotate_y(0.2)
    r = make_renderer()
    try:
        r.update(sc)
        (dp,) = on_device(moved)
        r.set_vertices(0, dp, recompute_normals=True)
        rebuilds = r.stats()["full_rebuilds"]
        sc.set_instance_transform(fan, shift)
        r.update_transforms(sc)  # (sc.vertices are still the undeformed ones: only the matrices go)
        assert r.stats()["full_rebuilds"] == rebuilds + 1
        assert np.array_equal(rows(r.read_vertices(0, n)), rows(ref.vertices))
        ref.set_instance_transform(fan, shift)
        got = render(r, cam)
        r.update(ref)
        same_frame(got, render(r, cam), "a fresh upload of the new vertices and transforms")
        # set_vertices, then the host's records over part of the range, then the rebuild
        sc2, _, _, _, ref2 = deformed_scene()
        r.update(sc2)
        r.set_vertices(0, dp, recompute_normals=True)
        first, count = names["grid"][0] - 6, 40  # from the Cornell box's last records through the grid into the fan
        part = deformed(ref2.vertices[first : first + count], 0.03, freq=4.0, phase=1.1)
        sc2.set_vertices(first, part)  # (everything outside the range is still the undeformed scene in the host's arrays)
        assert sc2.dirty_vertices == (first, first + count)
        r.update_vertices(sc2)
        combined = ref2.vertices.copy()
        combined[first : first + count] = part
        assert np.array_equal(rows(r.read_vertices(0, n)), rows(combined)) and not np.array_equal(rows(sc2.vertices), rows(combined))
        ref2.vertices[:] = combined
        same_frame(render(r, cam), _fresh(ref2, cam), "set_vertices then update_vertices: the combined records")
        sc2.set_instance_transform(fan, shift)
        r.update_transforms(sc2)
        assert np.array_equal(rows(r.read_vertices(0, n)), rows(combined))
        ref2.set_instance_transform(fan, shift)
        same_frame(render(r, cam), _fresh(ref2, cam), "... and after a rebuild from the kept scene")
    finally:
        r.close()


def _fresh(sc, cam, options=None):
    r = make_renderer(options=options)
    try:
        r.update(sc)
        return render(r, cam)
    finally:
        r.close()


@pytest.mark.gpu
def test_a_rigged_range_keeps_its_rest_pose(built):
    """Case 7: a rig over the grid, set_vertices over it, then animate: the records are those animate gives from the
    unchanged rest pose."""
    from test_animate import make_rig

    sc, _, names = streams_scene()
    first, count = names["grid"]
    rig, pose, expected = make_rig(sc.vertices, first, count, 2, 3, 7)
    p, nrm, uv = new_streams(sc, first, count, 51)
    r = make_renderer()
    try:
        r.update(sc)
        r.set_rigs([rig])
        r.set_vertices(first, *on_device(p, nrm, uv))
        assert np.array_equal(rows(r.read_vertices(first, count)), rows(packed(sc.vertices, first, p, nrm, uv)[first : first + count]))
        r.animate([pose])
        want = sc.vertices.copy()
        want[first : first + count] = expected
        assert np.array_equal(rows(r.read_vertices(0, sc.vertices.shape[0])), rows(want))
    finally:
        r.close()


@pytest.mark.gpu
def test_kept_first_hits_and_frames_in_flight(built):
    """Case 8: render, set_vertices, render: the second frame is a fresh context's (the kept first hits of the first are not
    used again). A render_async ticket submitted before the call completes with the old frame."""
    sc, cam, _, moved, ref = deformed_scene()
    r = make_renderer()
    try:
        r.update(sc)
        old = render(r, cam)
        same_frame(old, render(r, cam), "the same view again (kept first hits)")
        ticket = r.render_async(frame_of(cam), 0, 1)
        (dp,) = on_device(moved)
        r.set_vertices(0, dp, recompute_normals=True)
        same_frame(r.wait(ticket), old, "the ticket in flight")
        new = render(r, cam)
        assert not np.array_equal(new["radiance"], old["radiance"])
        same_frame(new, _fresh(ref, cam), "a fresh context")
    finally:
        r.close()


@pytest.mark.gpu
def test_refusals_change_nothing_and_name_the_field(built):
    """Case 9: every refusal of the header through the C ABI: -1, a message that names the field, the records and the frame
    as they were."""
    from stratum_amd.bdpt import BDPT

    sc, cam, _ = streams_scene()
    n = sc.vertices.shape[0]
    p, nrm, uv = new_streams(sc, 0, n, 61)
    stage = np.zeros(3 * n + 4, np.float32)
    r = BDPT(device=0)
    try:
        L, h = r._lib, r._h

        def desc(**kw):
            d = wire.VertexStreams()
            d.struct_size = C.sizeof(d)
            d.first_vertex, d.vertex_count = 0, n
            d.positions, d.position_stride = p.ctypes.data, 12
            for k, v in kw.items():
                setattr(d, k, v)
            return d

        info = wire.RefitInfo()
        assert L.sthip_scene_set_vertices(h, C.byref(desc()), C.byref(info)) == -1
        assert b"sthip_scene_upload" in L.sthip_last_error(h)
        r.update(sc)
        before = render(r, cam)
        cases = [
            ("struct_size", desc(struct_size=C.sizeof(wire.VertexStreams) - 4)),
            ("positions", desc(positions=None)),
            ("vertex_count", desc(vertex_count=n + 1)),
            ("vertex_count", desc(first_vertex=n, vertex_count=1)),
            ("vertex_count", desc(first_vertex=0xFFFFFFFF, vertex_count=2)),
            ("positions", desc(positions=stage.ctypes.data + 2)),
            ("normals", desc(normals=stage.ctypes.data + 1, normal_stride=12)),
            ("texcoords", desc(texcoords=stage.ctypes.data + 3, texcoord_stride=8)),
            ("position_stride", desc(position_stride=14)),
            ("normal_stride", desc(normals=nrm.ctypes.data, normal_stride=18)),
            ("texcoord_stride", desc(texcoords=uv.ctypes.data, texcoord_stride=10)),
            ("position_stride", desc(position_stride=8)),
            ("normal_stride", desc(normals=nrm.ctypes.data, normal_stride=8)),
            ("texcoord_stride", desc(texcoords=uv.ctypes.data, texcoord_stride=4)),
            ("recompute_normals", desc(normals=nrm.ctypes.data, normal_stride=12, recompute_normals=1)),
        ]
        for field, d in cases:
            assert L.sthip_scene_set_vertices(h, C.byref(d), C.byref(info)) == -1, field
            message = L.sthip_last_error(h).decode()
            assert message.startswith("sthip_scene_set_vertices") and field in message, (field, message)
        assert L.sthip_scene_set_vertices(h, None, None) == -1 and L.sthip_scene_set_vertices(None, C.byref(desc()), None) == -1
        assert np.array_equal(rows(r.read_vertices(0, n)), rows(sc.vertices))
        same_frame(render(r, cam), before, "after the refused calls")
        assert r.stats()["full_rebuilds"] == 0
        assert L.sthip_scene_set_vertices(h, C.byref(desc(first_vertex=n, vertex_count=0)), C.byref(info)) == 0  # an empty range is a no-op
        assert np.array_equal(rows(r.read_vertices(0, n)), rows(sc.vertices))
        same_frame(render(r, cam), before, "after an empty call")
        with pytest.raises(ValueError):
            r.set_vertices(0, p, normals=nrm[:-1])
        with pytest.raises(ValueError):
            r.set_vertices(0, p.astype(np.float64))
        assert L.sthip_scene_set_vertices(h, C.byref(desc(normals=nrm.ctypes.data, normal_stride=12, texcoords=uv.ctypes.data, texcoord_stride=8)), C.byref(info)) == 0
        assert np.array_equal(rows(r.read_vertices(0, n)), rows(packed(sc.vertices, 0, p, nrm, uv)))
    finally:
        r.close()


@pytest.mark.gpu
def test_normals_and_frames_with_poisoned_allocations(built):
    """Case 10: cases 4 and 5 with the default options once more in one fresh child process with STHIP_POISON_ALLOC (read once
    per process). The allocations of vertex_streams.hip honour it as DevBuf::ensure does: the adjacency's rows and slots, the
    face vectors' scratch and the staging of host streams start as 0x7F bytes, so a slot or a row read before a launch wrote it
    shows in the records or the frame the child compares."""
    if os.environ.get("STHIP_VERTEX_STREAMS_POISON_CHILD"):
        return  # (this is the child)
    env = dict(os.environ, STHIP_POISON_ALLOC="0x7F", STHIP_VERTEX_STREAMS_POISON_CHILD="1")
    out = subprocess.run(
        [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "recomputed_normals or (frames_equal and 0-1-1)"],
        env=env, cwd=ROOT, capture_output=True, text=True, timeout=600,
    )
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert re.search(r"\b2 passed", out.stdout) and "failed" not in out.stdout, out.stdout[-2000:]


# ---------------------------------------------------------------------------------------------------------------------------
# the C++ host
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vertex_streams_host(built):
    import __graft_entry__ as g

    exe = os.path.join(ROOT, "tests", "cpp", "vertex_streams_host")
    deps = [HOST_SRC, os.path.join(ROOT, "tests", "cpp", "scene_reader.hpp"), os.path.join(ROOT, "stratum_amd", "host", "stratum_hip.hpp"), g.LIB]
    if g._newer(exe, deps):
        rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
        subprocess.check_call(
            [CXX, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", exe, HOST_SRC]
            + ["-L" + os.path.dirname(g.LIB), "-lstratum_hip", "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-ldl", "-Wl,-rpath," + os.path.dirname(g.LIB), "-Wl,-rpath," + os.path.join(rocm, "lib")]
        )
    return exe


def test_cpp_host_with_the_device_vertex_call_builds(vertex_streams_host):
    """The C++ host with BDPT::set_vertices_device compiles and links against the library (no GPU needed); without arguments
    the program only prints its usage."""
    out = subprocess.run([vertex_streams_host], capture_output=True, text=True)
    assert out.returncode == 2 and "usage: vertex_streams_host" in out.stderr


@pytest.mark.gpu
def test_cpp_host_deforms_a_mesh_from_a_device_stream(vertex_streams_host, tmp_path):
    """tests/cpp/vertex_streams_host.cpp: the C++ host deforms a mesh through BDPT::update, through set_vertices_device from a
    hipMalloc'd stream and on a fresh host: the same frame bytes; a BDPT::update after the device call does not resurrect the
    vertices the bound scene held."""
    from stratum_amd.scene import dump_description

    sc, cam, _ = streams_scene()
    path = str(tmp_path / "scene.bin")
    dump_description(path, sc, frame_of(cam))
    out = subprocess.run([vertex_streams_host, path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "VERTEX STREAMS HOST OK" in out.stdout and "FAIL" not in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
