"""sthip_scene_set_transforms / sthip_scene_read_transforms / sthip_scene_read_top_level: instance transforms from host or
device memory, the derived inverse and motion matrices, and the top level built on the device (csrc/top_level.hip).

One tiny scene family: a 2-triangle quad instanced N times, a sphere light, a fog volume and a merged identity floor. Entry
counts 1, 2, 3, 64, 65, 257, 1025 (the wrapped leaf, the smallest trees, the tails of a wave and of a 256- and a 1024-thread
block); placements: a jittered grid, all at one transform (equal keys), collinear along x (zero extent on two axes), two
tight clusters 1e6 apart along the diagonal (the quantisation collapses each to one key), rotations with non-uniform scales.
The reference of the entry boxes is the host builder itself (tests/cpp/top_level_ref.cpp links bvh_build.cpp)."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from stratum_amd import camera, scene as scene_mod, wire
from stratum_amd.scene import SceneBuilder, rotate_x, rotate_y, scale, translate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = [1, 2, 3, 64, 65, 257, 1025]
PLACEMENTS = ["grid", "same", "collinear", "clusters", "rotscale"]
W, H, SEEDS = 64, 48, 2
CAM = {"eye": (0.0, 0.0, 3.9), "target": (0.0, 0.0, 0.0), "fovy": np.radians(39.3)}


def _fog():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "fog_sphere.npz"))["grid"]


def _quad():
    pos = np.array([(-0.5, -0.5, 0), (0.5, -0.5, 0), (0.5, 0.5, 0), (-0.5, 0.5, 0)], np.float32)
    nrm = np.tile(np.array((0, 0, 1), np.float32), (4, 1))
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    return pos, nrm, uv, np.array([[0, 1, 2], [0, 2, 3]])


def _plan(entries):
    """How `entries` top-level entries are made up: (quads, sphere, volume, floor)."""
    if entries >= 4:
        return entries - 3, True, True, True
    return {1: (1, False, False, False), 2: (1, True, False, False), 3: (2, True, False, False)}[entries]


def placement(kind, n, seed=7):
    """n object-to-world matrices (n, 4, 4) of the quads."""
    rng = np.random.default_rng(seed + n)
    side = int(np.ceil(np.sqrt(n)))
    step = 1.6 / side
    size = 0.35 * step
    out = []
    for k in range(n):
        gx, gy = (k % side + 0.5) * step - 0.8, (k // side + 0.5) * step - 0.8
        if kind == "grid":
            j = (rng.random(3) - 0.5) * 0.2 * step
            m = translate((gx + j[0], gy + j[1], 0.3 * j[2] / step)) @ scale((size, size, size))
        elif kind == "same":
            m = translate((0.1, -0.2, 0.05)) @ rotate_y(0.3) @ scale((0.4, 0.4, 0.4))
        elif kind == "collinear":
            m = translate(((k + 0.5) * (1.6 / n) - 0.8, 0.25, -0.125)) @ scale((0.5 * 1.6 / n,) * 3)
        elif kind == "clusters":
            # (a quarter-unit lattice and a power-of-two scale: every matrix and inverse is exact in binary32 at 1e6 too; a
            # cluster spans < 6 units, a cell of the 16-bit key grid over the 1e6 diagonal ~15)
            j, cs = k // 2, int(np.ceil(np.sqrt((n + 1) // 2)))
            base = 1.0e6 if k & 1 else 0.0
            m = translate((base + 0.25 * (j % cs), base + 0.25 * (j // cs), base)) @ scale((0.125, 0.125, 0.125))
        elif kind == "rotscale":
            s = size * np.array([0.5 + rng.random(), 0.3 + 0.7 * rng.random(), 1.0])
            m = translate((gx, gy, 0.1 * (rng.random() - 0.5))) @ rotate_y(0.6 * (rng.random() - 0.5)) @ rotate_x(0.6 * (rng.random() - 0.5)) @ scale(tuple(s))
        else:
            raise KeyError(kind)
        out.append(np.asarray(m, np.float64))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def family(entries):
    """(scene, indices of the quad instances, index of the sphere or None, index of the volume instance or None); shared."""
    return build_family(entries)


def build_family(entries):
    nq, sphere, volume, floor = _plan(entries)
    b = SceneBuilder("top_level_%d" % entries)
    white = b.add_material((0.73, 0.73, 0.73))
    lamp = b.add_emitter((18.0, 15.0, 10.0))
    mesh = b.add_mesh(*_quad())
    quads = [b.add_instance(mesh, white, m) for m in placement("grid", nq, seed=3)]
    if floor:
        p = np.array([(-1, -1, 1), (1, -1, 1), (1, -1, -1), (-1, -1, -1)], np.float32)
        b.add_instance(b.add_mesh(p, np.tile(np.array((0, 1, 0), np.float32), (4, 1)), _quad()[2], _quad()[3]), white)
    if sphere:
        b.add_sphere(lamp, 0.15, translate((0.0, 0.8, 0.6)))
    if volume:
        b.add_medium(b.add_volume(_fog()), density_scale=(3.0, 3.0, 3.0), albedo_scale=(0.9, 0.9, 0.9), transform=translate((0.2, 0.1, 0.9)) @ scale((0.4, 0.4, 0.4)))
    sc = b.build()
    types = sc.instances["packed"][:, 0] & 0xF
    n = sc.instances.shape[0]
    assert n == nq + int(floor) + int(sphere) + int(volume)
    want = placement("grid", nq, seed=3)[:, :3, :].astype(np.float32)
    assert np.array_equal(sc.transforms["m"][quads], want)  # (triangle instances keep the order they were added in)
    others = [i for i in range(n) if types[i] != types[quads[0]]]
    sph = others[0] if sphere else None
    vol = others[1] if volume else None
    return sc, quads, sph, vol


def moved(entries, kind):
    """The three arrays (n, 3, 4) float32 of the family's scene after the move `kind`: quads placed anew, the sphere and the
    volume shifted (their box formulas see a matrix that is not the uploaded one); motion = tmul(uploaded, new inverse)."""
    sc, quads, sph, vol = family(entries)
    xf = sc.transforms["m"].copy()
    xf[quads] = placement(kind, len(quads))[:, :3, :].astype(np.float32)
    if sph is not None:
        xf[sph][:, 3] += np.array((0.05, -0.1, 0.02), np.float32)
    if vol is not None:
        xf[vol][:, 3] += np.array((-0.1, 0.05, 0.03), np.float32)
    inv = np.stack([scene_mod.transform_inverse(m) for m in xf])
    motion = np.stack([scene_mod.tmul(p, i) for p, i in zip(sc.transforms["m"], inv)])
    return xf, inv, motion


def moved_scene(entries, kind):
    """A fresh scene object holding the moved arrays (what a host would upload instead of moving)."""
    sc = build_family(entries)[0]
    xf, inv, motion = moved(entries, kind)
    sc.transforms["m"][:], sc.inverse_transforms["m"][:], sc.motion_transforms["m"][:] = xf, inv, motion
    return sc


def as_td(a):
    out = np.zeros(a.shape[0], wire.TransformData)
    out["m"] = a
    return out


def old_call(r, xf, inv, motion):
    rc = r._lib.sthip_scene_update_transforms(r._h, wire.ptr(as_td(xf)), wire.ptr(as_td(inv)), wire.ptr(as_td(motion)), xf.shape[0])
    r._check(rc, "sthip_scene_update_transforms")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_frame(a, b, what=""):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(bits(np.asarray(a[k])), bits(np.asarray(b[k]))), (what, k)


def same_floats(a, b):
    """Bit equality of float32 arrays, +0 and -0 alike."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ua, ub = a.view(np.uint32).copy(), b.view(np.uint32).copy()
    ua[ua == 0x80000000] = 0
    ub[ub == 0x80000000] = 0
    return np.array_equal(ua, ub)


def make_renderer(options=None, flags=(), args=None):
    from stratum_amd.bdpt import BDPT

    r = BDPT(device=0, args=dict(args or {}, bdptFlag=list(flags)))
    for k, v in (options or {}).items():
        r.set_option(k, v)
    return r


def frame():
    return camera.Frame(W, H, CAM["fovy"], CAM["eye"], CAM["target"])


def dump_scene(d, sc):
    for arr, fn in ((sc.vertices, "vertices"), (sc.indices, "indices"), (sc.instances, "instances"), (sc.transforms, "xf"), (sc.inverse_transforms, "inv_xf"), (sc.materials, "materials")):
        np.ascontiguousarray(arr).tofile(os.path.join(d, fn + ".bin"))
    for k, v in enumerate(sc.volumes):
        np.ascontiguousarray(v).tofile(os.path.join(d, "volume%d.bin" % k))


def build_ref(exe, extra=()):
    csrc = os.path.join(ROOT, "stratum_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer", *extra, "-o", exe, os.path.join(ROOT, "tests", "cpp", "top_level_ref.cpp"),
                           os.path.join(csrc, "bvh_build.cpp"), "-lpthread"])
    return exe


def run_ref(exe, d, entries, kinds, env=None):
    """The host builder's boxes, centre and radius for the moves `kinds` of the family with `entries` entries."""
    os.makedirs(d, exist_ok=True)
    dump_scene(d, family(entries)[0])
    for kind in kinds:
        xf, inv, _ = moved(entries, kind)
        as_td(xf).tofile(os.path.join(d, kind + "_xf.bin"))
        as_td(inv).tofile(os.path.join(d, kind + "_inv.bin"))
    out = subprocess.run([exe, d] + list(kinds), capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    res = {}
    for kind in kinds:
        raw = np.fromfile(os.path.join(d, kind + "_ref.bin"), np.uint8)
        m = int(raw[:4].view(np.uint32)[0])
        f = raw[4 : 4 + 24 * m + 16].view(np.float32)
        tail = raw[4 + 24 * m + 16 :].view(np.uint32)
        res[kind] = {"boxes": f[: 6 * m].reshape(m, 2, 3), "center": f[6 * m : 6 * m + 3], "radius": f[6 * m + 3], "nodes": int(tail[0]), "world": int(tail[1])}
    return res


@pytest.fixture(scope="session")
def top_level_ref(tmp_path_factory):
    return build_ref(str(tmp_path_factory.mktemp("top_level_ref") / "top_level_ref"))


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_three_symbols():
    text = open(os.path.join(ROOT, "include", "sthip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int\s+sthip_scene_set_transforms\s*\(\s*sthip_ctx\s*\*\s*\w*\s*,\s*const\s+sthip_transforms_desc\s*\*\s*\w*\s*,\s*uint32_t\s+struct_size\s*,\s*sthip_transforms_info\s*\*\s*\w*\s*\)", text)
    assert re.search(r"int\s+sthip_scene_read_transforms\s*\(", text) and re.search(r"int\s+sthip_scene_read_top_level\s*\(", text)
    for name in ("sthip_transforms_desc", "sthip_transforms_info", "sthip_top_node"):
        assert "typedef struct " + name in text
    assert re.search(r"#define\s+STHIP_ABI_VERSION\s+11\b", text)


def test_library_exports_the_three_symbols(built):
    from stratum_amd import _lib

    for name in ("sthip_scene_set_transforms", "sthip_scene_read_transforms", "sthip_scene_read_top_level"):
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)


def test_wire_mirrors_have_the_layout_of_the_c_structs(tmp_path):
    fields = {"sthip_transforms_desc": ["transforms", "inverse_transforms", "motion_transforms", "instance_count", "device_ptr", "top_level", "derive_motion"],
              "sthip_transforms_info": ["device_ms", "total_ms", "top_level_nodes", "top_level_depth", "rebuilt", "builder_used"],
              "sthip_top_node": ["lo", "child0", "hi", "child1"]}
    body = "".join('  printf("%s %%zu", sizeof(%s));\n%s  printf("\\n");\n' % (s, s, "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (s, f) for f in fs)) for s, fs in fields.items())
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sthip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in subprocess.check_output([exe]).decode().splitlines()}
    d, i = wire.TransformsDesc, wire.TransformsInfo
    assert got["sthip_transforms_desc"] == [C.sizeof(d)] + [getattr(d, f).offset for f, _ in d._fields_] and C.sizeof(d) == wire.TRANSFORMS_DESC_BYTES
    assert [f for f, _ in d._fields_] == fields["sthip_transforms_desc"]
    assert got["sthip_transforms_info"] == [C.sizeof(i)] + [getattr(i, f).offset for f, _ in i._fields_]
    assert [f for f, _ in i._fields_] == fields["sthip_transforms_info"]
    t = wire.TopNode
    assert got["sthip_top_node"] == [t.itemsize] + [t.fields[f][1] for f in fields["sthip_top_node"]]


def test_reference_program_under_sanitizers(tmp_path):
    """tests/cpp/top_level_ref.cpp as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (host code
    only): every placement at 65 and at 3 entries; the boxes it reports contain the quads' transformed corners."""
    exe = build_ref(str(tmp_path / "top_level_ref_asan"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    for entries in (3, 65):
        res = run_ref(exe, str(tmp_path / ("n%d" % entries)), entries, PLACEMENTS, env=env)
        sc, quads, _, _ = family(entries)
        for kind in PLACEMENTS:
            ref = res[kind]
            assert ref["boxes"].shape[0] == entries and ref["world"] == 0 and ref["nodes"] >= 1
            xf = moved(entries, kind)[0]
            corners = np.array([(x, y, 0, 1) for x in (-0.5, 0.5) for y in (-0.5, 0.5)], np.float64)
            # (entry k of a scene without a merged mesh is instance k: quads first)
            for k in quads[:: max(1, len(quads) // 8)]:
                w = corners @ xf[k].astype(np.float64).T
                e = k + (1 if entries >= 4 else 0)  # (the merged mesh's entry comes first)
                assert (ref["boxes"][e, 0] <= w.min(0)).all() and (ref["boxes"][e, 1] >= w.max(0)).all(), (kind, k)
            assert np.isfinite(ref["radius"]) and ref["radius"] > 0


TOP_LEVEL_HOST = os.path.join(ROOT, "tests", "cpp", "top_level_host")


@pytest.fixture(scope="session")
def top_level_host(built):
    src = os.path.join(ROOT, "tests", "cpp", "top_level_host.cpp")
    deps = [src, os.path.join(ROOT, "tests", "cpp", "scene_reader.hpp"), os.path.join(ROOT, "stratum_amd", "host", "stratum_hip.hpp"), os.path.join(ROOT, "include", "sthip.h")]
    if not os.path.exists(TOP_LEVEL_HOST) or os.path.getmtime(TOP_LEVEL_HOST) < max(os.path.getmtime(d) for d in deps):
        rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
        lib = os.path.join(ROOT, "stratum_amd")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", TOP_LEVEL_HOST, src, "-L" + lib, "-lstratum_hip",
                               "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath," + os.path.join(rocm, "lib")])
    return TOP_LEVEL_HOST


def test_cpp_host_with_the_device_routes_builds(top_level_host):
    """The C++ host with Scene::set_top_level_on_device and BDPT::set_instance_transforms_device compiles and links against the
    library (no GPU needed); without arguments the program only prints its usage."""
    out = subprocess.run([top_level_host], capture_output=True, text=True)
    assert out.returncode == 2 and "usage: top_level_host" in out.stderr


@pytest.mark.gpu
def test_cpp_host_moves_instances_by_each_route(top_level_host, tmp_path):
    """Two moves of the Cornell box's blocks through the C++ host: the transforms-only branch of BDPT::update with the switch
    off and on, and the second move from device memory through set_instance_transforms_device: the same frames, byte for byte."""
    from stratum_amd import scenes
    from stratum_amd.scene import dump_description

    sc, cam = scenes.cornell_box()
    desc = str(tmp_path / "scene.bin")
    dump_description(desc, sc, camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"]))
    frames = {}
    for route in ("host", "device_builder", "device_ptr"):
        outp = str(tmp_path / (route + ".bin"))
        out = subprocess.run([top_level_host, desc, outp, "2", "0.05,0.0,-0.04", route], capture_output=True, text=True)
        want = "MOVED route=%s transforms_only=1 on_device=%d" % (route, 1 if route == "device_builder" else 0)
        assert out.returncode == 0 and want in out.stdout, out.stdout + out.stderr
        frames[route] = [np.fromfile(outp + s, np.uint8) for s in (".f2", ".f3")]
    assert not np.array_equal(frames["host"][0], frames["host"][1])
    for route in ("device_builder", "device_ptr"):
        for k in range(2):
            assert np.array_equal(frames[route][k], frames["host"][k]), (route, "frame %d" % (k + 2))


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
_renderers = {}


def renderer_for(entries):
    """One living context per entry count, uploaded with the family's scene (every move replaces all transforms)."""
    if entries not in _renderers:
        r = make_renderer()
        r.update(family(entries)[0])
        _renderers[entries] = r
    return _renderers[entries]


def tree_checks(top, info, entries):
    nodes, boxes, root = top["nodes"], top["entry_boxes"], top["root"]
    assert boxes.shape[0] == entries
    want_nodes = entries - 1 if entries >= 2 else 1
    assert len(nodes) == want_nodes == info["top_level_nodes"] and root == 0
    seen = np.zeros(entries, np.int64)
    height = 0
    stack = [(root, 1)]
    visited = set()
    while stack:
        k, depth = stack.pop()
        assert k not in visited and k < len(nodes)
        visited.add(k)
        height = max(height, depth)
        nd = nodes[k]
        for c in (int(nd["child0"]), int(nd["child1"])):
            if c & 0x80000000:
                e = c & 0x7FFFFFFF
                assert e < entries
                seen[e] += 1
                assert (nd["lo"] <= boxes[e, 0]).all() and (nd["hi"] >= boxes[e, 1]).all(), (k, e)
            else:
                assert (nd["lo"] <= nodes[c]["lo"]).all() and (nd["hi"] >= nodes[c]["hi"]).all(), (k, c)
                stack.append((c, depth + 1))
    assert len(visited) == want_nodes
    assert (seen == (2 if entries == 1 else 1)).all()  # (one entry: its leaf sits in both slots of the wrapping node)
    assert height <= info["top_level_depth"]


@pytest.mark.gpu
@pytest.mark.parametrize("entries", COUNTS)
def test_boxes_and_tree_of_the_device_builder(built, top_level_ref, tmp_path, entries):
    """Checks 1 and 2 for every placement: boxes, centre and radius have the host builder's bits; the nodes read back form a
    valid tree over all entries; a second call with the same input gives byte-equal nodes."""
    ref = run_ref(top_level_ref, str(tmp_path / "ref"), entries, PLACEMENTS)
    r = renderer_for(entries)
    for kind in PLACEMENTS:
        xf, inv, motion = moved(entries, kind)
        info = r.set_transforms(xf, inv, motion, top_level="device")
        assert info["builder_used"] == 1 and info["rebuilt"] == 0
        top = r.read_top_level()
        assert same_floats(top["entry_boxes"], ref[kind]["boxes"]), kind
        assert same_floats(top["center"], ref[kind]["center"]) and same_floats(np.float32(top["radius"]), ref[kind]["radius"]), kind
        tree_checks(top, info, entries)
        r.set_transforms(xf, inv, motion, top_level="device")
        again = r.read_top_level()
        assert bits(again["nodes"]).tobytes() == bits(top["nodes"]).tobytes() and again["root"] == top["root"], kind
        # after the host call the read call computes the boxes of the resident matrices again (the same kernel: the host call
        # keeps no boxes) and reads the host-built nodes: as many as the host builder made
        old_call(r, xf, inv, motion)
        host = r.read_top_level()
        assert same_floats(host["entry_boxes"], ref[kind]["boxes"]) and len(host["nodes"]) == ref[kind]["nodes"], kind


def rays_for(entries, kind, boxes=None, n_random=20000):
    """`boxes`: the entry boxes as read_top_level gives them (entries, 2, 3): rays along their edges and through their corners,
    where the outward rounding of the packed planes decides whether a walk enters a leaf."""
    sc, quads, _, _ = family(entries)
    xf = moved(entries, kind)[0].astype(np.float64)
    rays = []
    for k in quads:  # one ray per instance, aimed at its centre from just in front of it
        m = xf[k]
        c = m[:, 3]
        nrm = m[:, 2] / np.linalg.norm(m[:, 2])
        ext = np.linalg.norm(m[:, 0])
        o = c + nrm * (2.0 if kind == "clusters" else 0.25) * ext  # (clusters: a distance binary32 resolves at 1e6)
        rays.append((o, c - o))
    aimed = len(rays)
    for k in quads[:64]:  # along the edges and through the corners of the quads
        m = xf[k]
        p = [m[:, :3] @ np.array(q) + m[:, 3] for q in ((-0.5, -0.5, 0), (0.5, -0.5, 0), (0.5, 0.5, 0), (-0.5, 0.5, 0))]
        for a in range(4):
            d = p[(a + 1) % 4] - p[a]
            rays.append((p[a] - d, d))  # along an edge
            o = np.array(CAM["eye"], np.float64)
            rays.append((o, p[a] - o))  # through a corner
    if boxes is not None:
        pick = np.linspace(0, len(boxes) - 1, min(len(boxes), 48)).astype(int)  # (the first, the last, and entries between)
        for b in np.asarray(boxes, np.float64)[pick]:
            if not np.isfinite(b).all():
                continue
            corner = [np.array([b[(c >> a) & 1][a] for a in range(3)]) for c in range(8)]
            for c in range(8):
                for a in range(3):
                    if not (c >> a) & 1:  # the 12 edges: from one corner past the other, starting a length before it
                        d = corner[c | (1 << a)] - corner[c]
                        rays.append((corner[c] - d, d))
                o = np.array(CAM["eye"], np.float64)
                rays.append((o, corner[c] - o))  # through a corner of the box
    rng = np.random.default_rng(11)
    o = rng.uniform(-1.2, 1.2, (n_random, 3)) + np.array((0, 0, 1.5))
    t = rng.uniform(-0.9, 0.9, (n_random, 3)) * np.array((1, 1, 0.2))
    rays += list(zip(o, t - o))
    out = np.zeros(len(rays), wire.Ray)
    out["origin"] = np.array([r[0] for r in rays], np.float32)
    out["direction"] = np.array([r[1] for r in rays], np.float32)
    out["tmin"], out["tmax"] = 0.0, 1.0e9
    return out, aimed


def ray_checks(r, entries, kind):
    sc, quads, _, _ = family(entries)
    xf, inv, motion = moved(entries, kind)
    old_call(r, xf, inv, motion)
    rays, aimed = rays_for(entries, kind, r.read_top_level()["entry_boxes"])
    want = [r.trace(rays, any_hit=False), r.trace(rays, any_hit=True)]
    inst = want[0]["instance_primitive_index"][:aimed] & 0xFFFF
    expect = np.array([quads[0]] * aimed if kind == "same" else quads, np.uint32)  # (coincident instances: the lowest id)
    assert np.array_equal(inst, expect), (kind, "precondition: each aimed ray hits its instance")
    for builder, ptr in (("device", False), ("device", True), ("host", True)):
        if ptr:
            import torch

            t = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (xf, inv, motion)]
            torch.cuda.synchronize()
            r.set_transforms(*t, top_level=builder)
        else:
            r.set_transforms(xf, inv, motion, top_level=builder)
        got = [r.trace(rays, any_hit=False), r.trace(rays, any_hit=True)]
        assert bits(got[0]).tobytes() == bits(want[0]).tobytes(), (kind, builder, ptr, "closest")
        assert np.array_equal(got[1]["instance_primitive_index"], want[1]["instance_primitive_index"]), (kind, builder, ptr, "any")


@pytest.mark.gpu
@pytest.mark.parametrize("entries", COUNTS)
def test_rays_hit_what_the_host_built_top_level_gives(built, entries):
    """Check 3: closest and any hit, bit-equal to the same scene after sthip_scene_update_transforms with the same matrices."""
    r = renderer_for(entries)
    for kind in PLACEMENTS:
        ray_checks(r, entries, kind)


def frame_checks(entries, kind, options=None, flags=(), args=None):
    sc = family(entries)[0]
    xf, inv, motion = moved(entries, kind)
    fr = frame()
    a = make_renderer(options, flags, args)
    a.update(sc)
    before = a.render(fr, 0, SEEDS)
    old_call(a, xf, inv, motion)
    want = a.render(fr, 0, SEEDS)
    assert not np.array_equal(want["radiance"], before["radiance"])
    fresh = make_renderer(options, flags, args)
    fresh.update(moved_scene(entries, kind))
    same_frame(fresh.render(fr, 0, SEEDS), want, "fresh upload vs old call")
    fresh.close()
    import torch

    for builder in ("host", "device"):
        for ptr in (False, True):
            b = make_renderer(options, flags, args)
            b.update(sc)
            b.render(fr, 0, 1)  # (kept first hits and grids of the scene before the move)
            arrays = [torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (xf, inv, motion)] if ptr else [xf, inv, motion]
            info = b.set_transforms(*arrays, top_level=builder)
            assert info["builder_used"] == (1 if builder == "device" else 0)
            same_frame(b.render(fr, 0, SEEDS), want, (builder, ptr))
            b.close()
    a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("what,options,flags,args", [
    ("default", None, (), None),
    ("wide8", {"wide_bvh": 3}, (), None),
    ("treetop", {"treetop": 1}, (), None),
    ("media", None, (), {"maxDiffuseVertices": 3, "maxNullCollisions": 64}),
    ("reuse_first_hits", {"reuse_first_hits": 1}, (), None),
])
def test_frames_equal_the_old_call_and_a_fresh_upload(built, what, options, flags, args):
    """Check 4 at 65 entries (grid -> rotations and scales): all outputs and ray_count, both builders, both pointer kinds."""
    frame_checks(65, "rotscale", options, flags, args)


@pytest.mark.gpu
def test_derived_inverse_and_motion(built):
    """Check 5: read_transforms after inverse=None, derive_motion=True equals scene.transform_inverse / scene.tmul bit for bit,
    from host and from device memory, with both builders; two successive moves (the second motion uses the resident
    transform of the first); an identity gives back an identity."""
    import torch

    sc, quads, sph, vol = family(65)
    rng = np.random.default_rng(5)
    n = sc.instances.shape[0]

    def matrices(step):
        xf = sc.transforms["m"].copy()
        for j, k in enumerate(quads):
            s = 10.0 ** rng.uniform(-3, 3, 3) if j % 3 == 0 else np.array((0.05, 0.04, 0.03))
            m = translate(tuple(rng.uniform(-1, 1, 3))) @ rotate_y(rng.uniform(-3, 3)) @ rotate_x(rng.uniform(-3, 3)) @ scale(tuple(s))
            if j % 5 == 1:  # a shear
                sh = np.eye(4)
                sh[0, 1], sh[2, 0] = 0.7 + step, -0.4
                m = m @ sh
            xf[k] = np.asarray(m)[:3, :].astype(np.float32)
        xf[quads[2]] = np.eye(4, dtype=np.float32)[:3, :]  # an identity
        return xf

    for builder in ("device", "host"):
        for ptr in (False, True):
            r = make_renderer()
            r.update(sc)
            prev = sc.transforms["m"].copy()
            for step in range(2):
                xf = matrices(step)
                r.set_transforms(torch.from_numpy(xf).to("cuda:0") if ptr else xf, None, None, derive_motion=True, top_level=builder)
                got = r.read_transforms()
                inv = np.stack([scene_mod.transform_inverse(m) for m in xf])
                motion = np.stack([scene_mod.tmul(p, i) for p, i in zip(prev, inv)])
                assert bits(got[0]).tobytes() == bits(xf).tobytes(), (builder, ptr, step)
                assert bits(got[1]).tobytes() == bits(inv).tobytes(), (builder, ptr, step)
                assert bits(got[2]).tobytes() == bits(motion).tobytes(), (builder, ptr, step)
                assert bits(got[1][quads[2]]).tobytes() == bits(np.eye(4, dtype=np.float32)[:3, :]).tobytes()
                prev = xf
            r.close()
    assert n == 65


@pytest.mark.gpu
def test_refusals_change_nothing(built):
    """Check 6: every refused call leaves the frame as it was and names its cause; a moved merged instance with a kept scene
    rebuilds (rebuilt = 1) into the fresh upload's frame."""
    from stratum_amd._lib import StratumHipError

    sc, quads, sph, vol = family(65)
    xf, inv, motion = moved(65, "rotscale")
    fr = frame()
    floor = [i for i in range(sc.instances.shape[0]) if i not in quads and i not in (sph, vol)][0]
    for keep in (1, 0):
        r = make_renderer({"keep_scene": keep})
        r.update(sc)
        before = r.render(fr, 0, SEEDS)

        def refused(code, word, call):
            with pytest.raises(StratumHipError) as e:
                call()
            assert "(%d)" % code in str(e.value) and word in str(e.value), str(e.value)
            same_frame(r.render(fr, 0, SEEDS), before, word)

        INVALID, UNSUPPORTED = -1, -4  # STHIP_ERR_INVALID_ARGUMENT, STHIP_ERR_UNSUPPORTED
        for builder in ("host", "device"):
            refused(UNSUPPORTED, "instance count", lambda: r.set_transforms(xf[:-1], inv[:-1], motion[:-1], top_level=builder))
            refused(INVALID, "derive_motion", lambda: r.set_transforms(xf, inv, motion, derive_motion=True, top_level=builder))
            sing = xf.copy()
            sing[quads[5]][:, :3] = 0.0
            refused(INVALID, "no inverse", lambda: r.set_transforms(sing, None, None, top_level=builder))
        nan = xf.copy()
        nan[quads[7]][0, 3] = np.nan
        refused(INVALID, "not finite", lambda: r.set_transforms(nan, inv, motion, top_level="device"))
        d = wire.TransformsDesc()
        a = [as_td(x) for x in (xf, inv, motion)]
        d.transforms, d.inverse_transforms, d.motion_transforms, d.instance_count = a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, xf.shape[0]
        refused(INVALID, "struct_size", lambda: r._check(r._lib.sthip_scene_set_transforms(r._h, C.byref(d), C.sizeof(d) - 4, None), "set"))
        d.transforms = None
        refused(INVALID, "transforms is NULL", lambda: r._check(r._lib.sthip_scene_set_transforms(r._h, C.byref(d), C.sizeof(d), None), "set"))
        # a merged instance moves
        mv = xf.copy()
        mv[floor] = np.asarray(translate((0.0, -0.1, 0.0)))[:3, :].astype(np.float32)
        mvi = np.stack([scene_mod.transform_inverse(m) for m in mv])
        for builder in ("host", "device"):
            if keep:
                info = r.set_transforms(mv, mvi, motion, top_level=builder)
                assert info["rebuilt"] == 1
                s2 = build_family(65)[0]
                s2.transforms["m"][:], s2.inverse_transforms["m"][:], s2.motion_transforms["m"][:] = mv, mvi, motion
                fresh = make_renderer()
                fresh.update(s2)
                same_frame(r.render(fr, 0, SEEDS), fresh.render(fr, 0, SEEDS), "rebuilt")
                fresh.close()
                r.update(sc)
            else:
                refused(UNSUPPORTED, "merged", lambda: r.set_transforms(mv, mvi, motion, top_level=builder))
        r.close()


@pytest.mark.gpu
def test_stale_host_mirrors_are_fetched(built):
    """Check 7: after a device-pointer move the kept scene and the entries' inverses are older than the device's; the refit,
    the old call's rebuild of a merged instance and set_images must see the device's."""
    import torch

    sc, quads, sph, vol = family(65)
    xf, inv, motion = moved(65, "rotscale")
    fr = frame()
    floor = [i for i in range(sc.instances.shape[0]) if i not in quads and i not in (sph, vol)][0]
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (xf, inv, motion)]
    # (a) device-pointer move, then update_vertices
    verts = sc.vertices.copy()
    verts["position"][:4, 2] += np.array((0.0, 0.2, 0.0, -0.2), np.float32)  # (the quad mesh comes first)
    for builder in ("device", "host"):
        r = make_renderer()
        s1 = build_family(65)[0]
        r.update(s1)
        r.set_transforms(dev[0], None, None, derive_motion=True, top_level=builder)
        s1.set_vertices(0, verts[:4])
        r.update_vertices(s1)
        s2 = moved_scene(65, "rotscale")
        s2.set_vertices(0, verts[:4])
        s2.dirty_vertices = None
        fresh = make_renderer()
        fresh.update(s2)
        same_frame(r.render(fr, 0, SEEDS), fresh.render(fr, 0, SEEDS), ("update_vertices", builder))
        # (b) then the old call moves a merged instance: the rebuild takes the right matrices and vertices
        mv = xf.copy()
        mv[floor] = np.asarray(translate((0.0, -0.1, 0.0)))[:3, :].astype(np.float32)
        mvi = np.stack([scene_mod.transform_inverse(m) for m in mv])
        old_call(r, mv, mvi, motion)
        s2.transforms["m"][:], s2.inverse_transforms["m"][:] = mv, mvi
        fresh.update(s2)
        same_frame(r.render(fr, 0, SEEDS), fresh.render(fr, 0, SEEDS), ("merged rebuild", builder))
        r.close()
        fresh.close()
    # (c) device-pointer move, then a layout rebuilt from the kept scene by update_vertices (wide_bvh = 3)
    r = make_renderer({"wide_bvh": 3})
    s1 = build_family(65)[0]
    r.update(s1)
    r.set_transforms(*dev, top_level="device")
    s1.set_vertices(0, verts[:4])
    assert r.update_vertices(s1)["rebuilt"] == 1
    s2 = moved_scene(65, "rotscale")
    s2.set_vertices(0, verts[:4])
    fresh = make_renderer({"wide_bvh": 3})
    fresh.update(s2)
    same_frame(r.render(fr, 0, SEEDS), fresh.render(fr, 0, SEEDS), "kept rebuild")
    r.close()
    fresh.close()


@pytest.mark.gpu
def test_device_move_then_set_images(built):
    """Check 7, third part: a device-pointer move followed by set_images renders the moved scene with the new texels."""
    import torch

    from stratum_amd import scenes

    sc, _ = scenes.textured_box()
    fr = camera.Frame(W, H, np.radians(39.3), (0.0, 0.0, 3.9), (0.0, 0.0, 0.0))
    n = sc.instances.shape[0]
    movable = [i for i in range(n) if not np.array_equal(sc.transforms["m"][i], np.eye(4, dtype=np.float32)[:3, :])]
    if not movable:
        pytest.fail("the textured box has no transformed instance to move")
    s2, _ = scenes.textured_box()
    for i in movable:
        m = np.vstack([sc.transforms["m"][i], [0, 0, 0, 1]]).astype(np.float64)
        s2.set_instance_transform(i, translate((0.05, 0.0, -0.04)) @ m)
    img = sc.images[0].copy()
    img[..., :3] = img[..., :3][..., ::-1]
    r = make_renderer()
    r.update(sc)
    r.set_transforms(torch.from_numpy(s2.transforms["m"].copy()).to("cuda:0"), None, None, derive_motion=True, top_level="device")
    r.set_images({0: img})
    s2.images[0] = img
    fresh = make_renderer()
    fresh.update(s2)
    same_frame(r.render(fr, 0, SEEDS), fresh.render(fr, 0, SEEDS), "set_images after a device move")
    r.close()
    fresh.close()


@pytest.mark.gpu
def test_poisoned_allocations(built):
    """Check 8: rays and frames at 65 and 257 entries once more in a fresh child process with STHIP_POISON_ALLOC=0x7F: the
    staging and scratch of top_level.hip start as 0x7F bytes, so anything read before a launch wrote it shows."""
    if os.environ.get("STHIP_TOP_LEVEL_POISON_CHILD"):
        return  # (this is the child)
    env = dict(os.environ, STHIP_POISON_ALLOC="0x7F", STHIP_TOP_LEVEL_POISON_CHILD="1")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "poison_child"],
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "passed" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("entries", [65, 257])
def test_poison_child_rays_and_frames(built, entries):
    """What test_poisoned_allocations runs in its child (and the parent runs unpoisoned)."""
    r = make_renderer()
    r.update(family(entries)[0])
    for kind in ("grid", "same", "rotscale"):
        ray_checks(r, entries, kind)
    r.close()
    frame_checks(entries, "rotscale")
