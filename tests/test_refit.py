"""Deforming meshes: sthip_scene_update_vertices replaces vertex records and refits the resident bottom levels on the device
(stratum_amd/csrc/refit.hip). Closest hit is the minimum over all triangles with ties broken by id, so a frame does not
depend on the shape of the tree: a refitted scene must give, bit for bit, the frame of a fresh upload of the deformed scene
and the oracle's frame of the deformed scene rendered from scratch."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from stratum_amd import camera, scenes, wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFORM_HOST = os.path.join(ROOT, "tests", "cpp", "deform_host")


# ---------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------
def deformed(vertices, amp, freq=3.0, phase=0.0):
    """A smooth finite displacement of packed vertices: a sine of position; normals tilted with it and re-normalised."""
    v = vertices.copy()
    p = v["position"].astype(np.float64)
    v["position"] = (p + amp * np.sin(freq * p[:, [1, 2, 0]] + phase)).astype(np.float32)
    n = v["normal"].astype(np.float64)
    n = n + 0.5 * amp * freq * np.cos(freq * p[:, [2, 0, 1]] + phase)
    length = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where(length > 1e-12, n / np.maximum(length, 1e-12), v["normal"].astype(np.float64))
    v["normal"] = n.astype(np.float32)
    assert np.isfinite(v["position"]).all() and np.isfinite(v["normal"]).all()
    return v


def deform(sc, amp, first=0, count=None, freq=3.0, phase=0.0):
    count = sc.vertices.shape[0] - first if count is None else count
    sc.set_vertices(first, deformed(sc.vertices[first : first + count], amp, freq, phase))


def mesh_range(sc, instance):
    """(first vertex, count) of the vertex records the triangles of `instance` refer to."""
    inst = sc.instances["packed"][instance]
    prims, stride = int((inst[1] >> 12) & 0xFFFF), int(inst[1] >> 28)
    off = int(inst[3])
    idx = np.frombuffer(sc.indices[off : off + 3 * prims * stride].tobytes(), dtype="<u2" if stride == 2 else "<u4").astype(np.int64)
    return int(inst[2]) + int(idx.min()), int(idx.max() - idx.min()) + 1


def same_frame(a, b, what=""):
    for k in ("radiance", "albedo", "prev_uv"):
        assert np.array_equal(a[k].view(np.uint32 if a[k].dtype.itemsize == 4 else np.uint16), b[k].view(np.uint32 if b[k].dtype.itemsize == 4 else np.uint16)), (what, k)
    assert np.array_equal(a["visibility"]["instance_primitive_index"], b["visibility"]["instance_primitive_index"]), (what, "visibility")
    assert np.array_equal(a["ray_count"], b["ray_count"]), (what, "ray_count")


def oracle_frame(sc, r, frame, seed_begin, seed_count):
    from oracle import oracle_py

    return oracle_py.OracleScene(sc).render(frame, r.push_constants(frame), r.mSamplingFlags, seed_begin, seed_count)


def _fog():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "fog_sphere.npz"))["grid"]


def make_renderer(args=None, flags=(), options=None):
    from stratum_amd.bdpt import BDPT

    r = BDPT(device=0, args=dict(args or {}, bdptFlag=list(flags)))
    for k, v in (options or {}).items():
        r.set_option(k, v)
    return r


SCENES = {
    "cornell": (lambda: scenes.cornell_box(), {}, []),
    "spheres_room": (lambda: scenes.spheres_room(), {"maxDiffuseVertices": 3}, []),
    "forest": (lambda: scenes.forest(n_instances=30, tree_tris=600, tree_kinds=2), {}, []),
    "fog": (lambda: scenes.cornell_box(fog=_fog()), {"maxDiffuseVertices": 3}, []),
    "textured": (lambda: scenes.textured_box(), {}, []),
    "alpha": (lambda: scenes.foliage(), {}, ["alphatest"]),
}


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_library_exports_update_vertices(built):
    from stratum_amd import _lib

    assert "sthip_scene_update_vertices" in _lib.EXPORTS
    assert hasattr(_lib.lib(), "sthip_scene_update_vertices")


def test_refit_info_mirror_has_the_size_of_the_c_struct(built, tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "sthip.h"\nint main(void) { printf("%zu\\n", sizeof(sthip_refit_info)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)])
    size = int(subprocess.check_output([exe]).decode())
    assert size == C.sizeof(wire.RefitInfo) == wire.REFIT_INFO_BYTES
    assert [f for f, _ in wire.RefitInfo._fields_] == ["device_ms", "total_ms", "sah_cost", "sah_cost_at_build", "rebuilt", "pad"]


def test_header_declares_update_vertices():
    text = open(os.path.join(ROOT, "include", "sthip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int\s+sthip_scene_update_vertices\s*\(\s*sthip_ctx\s*\*\s*\w*\s*,\s*const\s+sthip_PackedVertexData\s*\*\s*\w*\s*,\s*uint32_t\s+first_vertex\s*,\s*uint32_t\s+vertex_count\s*,\s*sthip_refit_info\s*\*\s*\w*\s*\)", text)
    assert "typedef struct sthip_refit_info" in text


def test_set_vertices_round_trips_and_tracks_the_dirty_range():
    sc, _ = scenes.cornell_box()
    assert sc.dirty_vertices is None
    before = sc.vertices.copy()
    part = deformed(sc.vertices[5:9], 0.1)
    sc.set_vertices(5, part)
    assert sc.dirty_vertices == (5, 9)
    assert np.array_equal(sc.vertices[5:9].tobytes(), part.tobytes()) and sc.vertices[:5].tobytes() == before[:5].tobytes() and sc.vertices[9:].tobytes() == before[9:].tobytes()
    sc.set_vertices(20, deformed(sc.vertices[20:22], 0.1))
    assert sc.dirty_vertices == (5, 22)
    sc.set_vertices(2, sc.vertices[2:3])
    assert sc.dirty_vertices == (2, 22)
    with pytest.raises(ValueError):
        sc.set_vertices(sc.vertices.shape[0] - 1, sc.vertices[:2])
    sc.dirty_vertices = None
    assert sc.dirty_vertices is None
    assert sc.desc().vertex_count == before.shape[0]


def test_product_still_never_touches_the_oracle():
    from test_abi import test_product_never_touches_the_oracle as check  # the existing test, over the tree with refit.hip in it

    check()
    assert os.path.exists(os.path.join(ROOT, "stratum_amd", "csrc", "refit.hip"))


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("builder", [0, 1])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_refit_gives_the_frame_of_a_fresh_upload_and_of_the_oracle(built, name, builder):
    """Render, deform every vertex, update_vertices, render: the frame is the oracle's on the deformed scene and the one a
    fresh upload gives, and not the frame before; the call refitted (rebuilt == 0, full_rebuilds unchanged)."""
    make, args, flags = SCENES[name]
    sc, cam = make()
    r = make_renderer(args, flags, {"bvh_builder": builder})
    try:
        r.update(sc)
        frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
        before = r.render(frame, 0, 2)
        rebuilds = r.stats()["full_rebuilds"]
        deform(sc, 0.04)
        info = r.update_vertices(sc)
        print(name, builder, info)
        assert info["rebuilt"] == 0 and r.stats()["full_rebuilds"] == rebuilds
        assert info["sah_cost"] > 0 and info["sah_cost_at_build"] > 0 and info["device_ms"] > 0 and info["total_ms"] >= info["device_ms"] * 0.5
        assert sc.dirty_vertices is None
        got = r.render(frame, 0, 2)
        same_frame(got, oracle_frame(sc, r, frame, 0, 2), "oracle")
        assert not np.array_equal(before["radiance"], got["radiance"])
        r.update(sc)
        same_frame(got, r.render(frame, 0, 2), "fresh upload")
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("builder", [0, 1])
def test_merged_transformed_and_emissive_meshes(built, builder):
    """Partial ranges in a multi-mesh scene: the floor (part of the merged world-space mesh), a box (a transformed
    instance), the ceiling light and an emissive panel under a transform (the emitter bounds must follow: answer_last_rays on
    and off give the same frame and ray counts, and the filter still answers rays), and a mesh pushed past the old scene bounds
    (centre and radius must follow)."""
    from stratum_amd.scene import rotate_y, scale, translate

    sc0, cam = scenes.cornell_box()
    b = sc0.builder
    glow = b.add_emitter((3.0, 6.0, 9.0))
    panel = b.add_mesh(*scenes.grid_surface(lambda u, v: np.stack([u - 0.5, 0.0 * u, v - 0.5], -1), 5, 5, flip=True))
    b.add_instance(panel, glow, translate((0.55, -0.2, 0.1)) @ rotate_y(0.7) @ scale((0.3, 1.0, 0.5)))
    sc = b.build()
    ident = [np.array_equal(m, np.eye(4, dtype=np.float32)[:3]) for m in sc.transforms["m"]]
    box = ident.index(False)
    lights = [int(i) for i in sc.lights]
    assert len(lights) == 2 and ident[lights[0]] and not ident[lights[1]] and ident[0]
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    steps = [("floor", 0, 0.06, 0.0), ("box", box, 0.08, 0.0), ("ceiling light", lights[0], 0.1, 0.7), ("panel", lights[1], 0.2, 0.3), ("floor past the bounds", 0, 0.0, 0.0)]
    r = make_renderer(options={"bvh_builder": builder})
    try:
        r.update(sc)
        prev = r.render(frame, 0, 2)
        for what, instance, amp, phase in steps:
            first, count = mesh_range(sc, instance)
            assert count < sc.vertices.shape[0]
            if what == "floor past the bounds":  # down and outward, far outside the box the scene had
                v = sc.vertices[first : first + count].copy()
                v["position"][:, 1] -= np.float32(0.8)
                v["position"][:, [0, 2]] *= np.float32(1.7)
                sc.set_vertices(first, v)
            else:
                deform(sc, amp, first, count, phase=phase)
            assert sc.dirty_vertices == (first, first + count)
            assert r.update_vertices(sc)["rebuilt"] == 0
            got = r.render(frame, 0, 2)
            assert r.stats()["rays_answered"] > 0, what
            same_frame(got, oracle_frame(sc, r, frame, 0, 2), what)
            r.set_option("answer_last_rays", 0)
            plain = r.render(frame, 0, 2)
            assert r.stats()["rays_answered"] == 0
            r.set_option("answer_last_rays", 1)
            same_frame(got, plain, what + ", every last ray traced")
            assert not np.array_equal(prev["radiance"], got["radiance"]), what
            prev = got
        r.update(sc)
        same_frame(prev, r.render(frame, 0, 2), "fresh upload")
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [1, 0, 2])
@pytest.mark.parametrize("builder", [0, 1])
def test_trace_contract_on_a_deformed_atrium(built, wide, builder):
    """BDPT.trace, closest and any hit, against the oracle's brute force on a deformed atrium of reduced size, with rays
    aimed at vertices and edges of the deformed triangles, through each form the boxes are walked in."""
    from oracle import oracle_py
    from test_gpu_parity import edge_rays, random_rays

    sc, _ = scenes.atrium(target_tris=40000)
    r = make_renderer(options={"bvh_builder": builder, "wide_bvh": wide})
    try:
        r.update(sc)
        deform(sc, 0.15, freq=1.3)
        info = r.update_vertices(sc)
        assert info["rebuilt"] == 0
        o = oracle_py.OracleScene(sc)
        rays = np.concatenate([random_rays(20000, 2, [-14, 0.2, -5.5], [14, 9.5, 5.5]), edge_rays(sc, 6000, 3)])
        got = r.trace(rays)
        ref, _ = o.trace(rays)
        for f in ("instance_primitive_index", "t", "b1", "b2"):
            assert np.array_equal(got[f].view(np.uint32), ref[f].view(np.uint32)), f
        sub = np.concatenate([rays[:300], rays[-300:]])
        ref_b, _ = o.trace(sub, brute=True)
        got_b = r.trace(sub)
        for f in ("instance_primitive_index", "t", "b1", "b2"):
            assert np.array_equal(got_b[f].view(np.uint32), ref_b[f].view(np.uint32)), f
        rays["tmax"] = 3.0
        sub = np.concatenate([rays[:300], rays[-300:]])
        got = r.trace(sub, any_hit=True)
        ref, _ = o.trace(sub, any_hit=True, brute=True)
        assert np.array_equal(got["instance_primitive_index"], ref["instance_primitive_index"])
        got = r.trace(rays, any_hit=True)
        ref, _ = o.trace(rays, any_hit=True)
        assert np.array_equal(got["instance_primitive_index"], ref["instance_primitive_index"])
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("builder", [0, 1])
def test_chains_of_refits(built, builder):
    """Ten small deformations with a refit each end in the frame of a fresh upload (another context's) and of the oracle; a second refit over the same vertices
    changes neither the cost (the outward rounding of the packed planes does not compound) nor the frame; restoring the vertices
    restores the frame; refits interleave with update_transforms, also with one that has to rebuild from the kept scene."""
    from stratum_amd.scene import rotate_y, scale, translate

    sc, cam = scenes.cornell_box()
    original = sc.vertices.copy()
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    r = make_renderer(options={"bvh_builder": builder})
    try:
        r.update(sc)
        first_frame = r.render(frame, 0, 2)
        at_build = None
        for k in range(10):
            deform(sc, 0.012, phase=0.37 * k, freq=2.0 + 0.3 * k)
            info = r.update_vertices(sc)
            assert info["rebuilt"] == 0
            at_build = info["sah_cost_at_build"] if at_build is None else at_build
            assert info["sah_cost_at_build"] == at_build  # (of the tree as built: the same figure every time)
        tenth = r.render(frame, 0, 2)
        cost = info["sah_cost"]
        for _ in range(2):  # the same vertices again, twice
            sc.set_vertices(0, sc.vertices.copy())
            again = r.update_vertices(sc)
            assert again["sah_cost"] == cost and again["rebuilt"] == 0
            same_frame(tenth, r.render(frame, 0, 2), "refit over the same vertices")
        same_frame(tenth, oracle_frame(sc, r, frame, 0, 2), "oracle after ten refits")
        fresh = make_renderer(options={"bvh_builder": builder})  # (another context: `r` keeps the tree it was built with, for what follows)
        try:
            fresh.update(sc)
            same_frame(tenth, fresh.render(frame, 0, 2), "fresh upload after ten refits")
        finally:
            fresh.close()
        assert r.stats()["full_rebuilds"] == 0
        # back to the original vertices: the original frame, and the cost the tree was built with
        sc.set_vertices(0, original)
        back = r.update_vertices(sc)
        same_frame(first_frame, r.render(frame, 0, 2), "restored")
        assert abs(back["sah_cost"] - back["sah_cost_at_build"]) <= 1e-5 * back["sah_cost_at_build"]
        # a transformed instance moves, then a mesh deforms, then the instance moves again
        ident = [np.array_equal(m, np.eye(4, dtype=np.float32)[:3]) for m in sc.transforms["m"]]
        box = ident.index(False)
        sc.set_instance_transform(box, translate((0.1, -1.0, 0.45)) @ rotate_y(0.6) @ scale((0.5, 0.7, 0.5)))
        r.update_transforms(sc)
        deform(sc, 0.05, phase=0.4)
        assert r.update_vertices(sc)["rebuilt"] == 0
        same_frame(r.render(frame, 0, 2), oracle_frame(sc, r, frame, 0, 2), "moved, then deformed")
        sc.set_instance_transform(box, translate((-0.2, -1.0, 0.3)) @ rotate_y(-0.3) @ scale((0.5, 0.9, 0.5)))
        r.update_transforms(sc)
        same_frame(r.render(frame, 0, 2), oracle_frame(sc, r, frame, 0, 2), "deformed, then moved")
        # an instance of the merged mesh moves: the scene is built again from the kept copy, which must hold the deformed vertices
        sc.set_instance_transform(0, translate((0.0, 0.1, 0.0)))
        r.update_transforms(sc)
        assert r.stats()["full_rebuilds"] == 1
        got = r.render(frame, 0, 2)
        same_frame(got, oracle_frame(sc, r, frame, 0, 2), "rebuilt from the kept scene")
        # ... and the rebuilt tree refits
        deform(sc, 0.03, phase=1.1)
        assert r.update_vertices(sc)["rebuilt"] == 0 and r.stats()["full_rebuilds"] == 1
        same_frame(r.render(frame, 0, 2), oracle_frame(sc, r, frame, 0, 2), "refit of the rebuilt tree")
    finally:
        r.close()


ESTIMATORS = [
    ("light tracing", lambda: scenes.cornell_box(), ["connecttoviews"], {}),
    ("connections", lambda: scenes.cornell_box(), ["connecttolightpaths", "~defershadowrays"], {"maxDiffuseVertices": 3, "maxPathVertices": 6}),
    ("lvc", lambda: scenes.cornell_box(), ["connecttolightpaths", "lightvertexcache", "lvcreservoirs"], {"lightPathCount": 4000, "reservoirM": 3, "maxDiffuseVertices": 3, "maxPathVertices": 6}),
    ("media", lambda: scenes.cornell_box(fog=_fog()), ["connecttoviews"], {"maxDiffuseVertices": 3}),
]


@pytest.mark.gpu
@pytest.mark.parametrize("what,make,flags,args", ESTIMATORS, ids=[e[0] for e in ESTIMATORS])
def test_estimators_on_a_refitted_scene(built, what, make, flags, args):
    """Light tracing, connections, the light vertex cache and media over a refitted scene."""
    sc, cam = make()
    frame = camera.Frame(100, 76, cam["fovy"], cam["eye"], cam["target"])
    r = make_renderer(args, flags, {"bvh_builder": 1})
    try:
        r.update(sc)
        before = r.render(frame, 0, 2)
        deform(sc, 0.05)
        assert r.update_vertices(sc)["rebuilt"] == 0
        got = r.render(frame, 0, 2)
        same_frame(got, oracle_frame(sc, r, frame, 0, 2), what)
        assert not np.array_equal(before["radiance"], got["radiance"])
    finally:
        r.close()


@pytest.mark.gpu
def test_kept_reservoir_grids_are_dropped(built):
    """NEE reservoirs with reuse and reuse_grids_persist = 1: the grids the frame before the deformation left name lights
    and positions of the old geometry; the call drops them, so the next call starts a new chain (the oracle's one-seed frame)."""
    flags, args = ["neereservoirs", "neereservoirreuse"], {"reservoirM": 2}
    sc, cam = scenes.cornell_box()
    frame = camera.Frame(100, 76, cam["fovy"], cam["eye"], cam["target"])
    r = make_renderer(args, flags, {"reuse_grids_persist": 1})
    try:
        r.update(sc)
        r.render(frame, 0, 1)
        chained = r.render(frame, 1, 1)  # looks into the grid seed 0 left
        deform(sc, 0.05)
        r.update_vertices(sc)
        got = r.render(frame, 1, 1)
        same_frame(got, oracle_frame(sc, r, frame, 1, 1), "a new chain after the refit")
        assert not np.array_equal(got["radiance"], chained["radiance"])
        after = r.render(frame, 2, 1)  # ... which goes on from there
        from oracle import oracle_py

        two = oracle_py.OracleScene(sc).render(frame, r.push_constants(frame), r.mSamplingFlags, 1, 2)
        assert np.array_equal(after["ray_count"] + got["ray_count"], two["ray_count"])
    finally:
        r.close()


@pytest.mark.gpu
def test_half_precision_and_frames_in_flight(built):
    """Half colour precision over a refitted scene; render_async: a ticket in flight when update_vertices is called
    completes with the old geometry, the next ticket shows the new one."""
    sc, cam = scenes.cornell_box()
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    r = make_renderer(options={"bvh_builder": 1})
    try:
        r.set_half_color_precision(True)
        r.update(sc)
        old = r.render(frame, 0, 2)
        assert old["radiance"].dtype == np.float16
        ticket = r.render_async(frame, 0, 2)
        deform(sc, 0.05)
        assert r.update_vertices(sc)["rebuilt"] == 0
        in_flight = r.wait(ticket)
        same_frame(in_flight, old, "the ticket in flight")
        new = r.wait(r.render_async(frame, 0, 2))
        assert not np.array_equal(new["radiance"], old["radiance"])
        same_frame(new, r.render(frame, 0, 2), "async against sync")
        r.update(sc)
        same_frame(new, r.render(frame, 0, 2), "fresh upload, half precision")
        r.set_half_color_precision(False)
        full = r.render(frame, 0, 2)
        same_frame(full, oracle_frame(sc, r, frame, 0, 2), "binary32 again")
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [{"embed_leaves": 1}, {"treetop": 1}, {"wide_bvh": 3}])
def test_layouts_the_refit_does_not_serve(built, layout):
    """embed_leaves, treetop, wide_bvh = 3: the frame is right whichever route the call took; with keep_scene = 0 the call
    either refits or is refused as unsupported, and the old scene then renders as before."""
    from stratum_amd._lib import StratumHipError

    sc, cam = scenes.cornell_box()
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    r = make_renderer(options=layout)
    try:
        r.update(sc)
        before = r.render(frame, 0, 2)
        rebuilds = r.stats()["full_rebuilds"]
        deform(sc, 0.05)
        info = r.update_vertices(sc)
        assert r.stats()["full_rebuilds"] == rebuilds + info["rebuilt"]
        got = r.render(frame, 0, 2)
        same_frame(got, oracle_frame(sc, r, frame, 0, 2), str(layout))
        assert not np.array_equal(before["radiance"], got["radiance"])
    finally:
        r.close()
    sc, cam = scenes.cornell_box()
    r = make_renderer(options=dict(layout, keep_scene=0))
    try:
        r.update(sc)
        before = r.render(frame, 0, 2)
        deform(sc, 0.05)
        try:
            info = r.update_vertices(sc)
            assert info["rebuilt"] == 0
            same_frame(r.render(frame, 0, 2), oracle_frame(sc, r, frame, 0, 2), "refitted without a kept scene")
        except StratumHipError as e:
            assert "(-4)" in str(e) and "keep_scene" in str(e), str(e)  # STHIP_ERR_UNSUPPORTED
            same_frame(r.render(frame, 0, 2), before, "refused: the old scene")
            assert r.stats()["full_rebuilds"] == 0
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [{"wide_bvh": 3}, {"embed_leaves": 1}])
def test_rebuild_from_the_kept_scene_sees_moved_instances(built, layout):
    """A layout that is built again from the kept scene, after a transforms-only update: the rebuild must find the instance
    where update_transforms put it, not where the upload had it."""
    from stratum_amd.scene import rotate_y, scale, translate

    sc, cam = scenes.cornell_box()
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    ident = [np.array_equal(m, np.eye(4, dtype=np.float32)[:3]) for m in sc.transforms["m"]]
    box = ident.index(False)
    r = make_renderer(options=layout)
    try:
        r.update(sc)
        sc.set_instance_transform(box, translate((0.1, -1.0, 0.45)) @ rotate_y(0.6) @ scale((0.5, 0.7, 0.5)))
        r.update_transforms(sc)
        rebuilds = r.stats()["full_rebuilds"]
        deform(sc, 0.05)
        info = r.update_vertices(sc)
        assert r.stats()["full_rebuilds"] == rebuilds + info["rebuilt"]
        same_frame(r.render(frame, 0, 2), oracle_frame(sc, r, frame, 0, 2), str(layout))
    finally:
        r.close()


@pytest.mark.gpu
def test_default_layout_refits_without_a_kept_scene(built):
    sc, cam = scenes.cornell_box()
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    r = make_renderer(options={"keep_scene": 0})
    try:
        r.update(sc)
        deform(sc, 0.05)
        assert r.update_vertices(sc)["rebuilt"] == 0
        same_frame(r.render(frame, 0, 2), oracle_frame(sc, r, frame, 0, 2), "keep_scene = 0")
    finally:
        r.close()


@pytest.mark.gpu
def test_refit_with_poisoned_allocations(built):
    """The basic case and the chains once more in a fresh child process with STHIP_POISON_ALLOC (read once per process). The
    refit's own allocations honour it as DevBuf::ensure does (refit.hip: refit_malloc, refit_host_malloc): its scratch boxes and
    heights, the schedule and its lists, marks, counts and offsets, the roots' and emitters' records and the pinned read-back
    staging all start as 0x7F bytes instead of the zero pages of a fresh process. A box, a height or a cost read before a
    launch wrote it is then 3.4e38 or 0x7F7F7F7F, not 0, and the frame or the cost the child compares comes out wrong."""
    if os.environ.get("STHIP_REFIT_POISON_CHILD"):
        return  # (this is the child)
    env = dict(os.environ, STHIP_POISON_ALLOC="0x7F", STHIP_REFIT_POISON_CHILD="1")
    out = subprocess.run(
        [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "(fresh_upload and (forest or cornell)) or chains"],
        env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500,
    )
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "failed" not in out.stdout


@pytest.mark.gpu
def test_argument_errors_are_refused_with_a_message(built):
    """Before a scene, a NULL pointer, a range past vertex_count: STHIP_ERR_INVALID_ARGUMENT with a message, and the scene
    renders as before."""
    from stratum_amd.bdpt import BDPT

    sc, cam = scenes.cornell_box()
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    r = BDPT(device=0)
    try:
        L, h = r._lib, r._h
        n = sc.vertices.shape[0]
        info = wire.RefitInfo()
        assert L.sthip_scene_update_vertices(h, wire.ptr(sc.vertices), 0, n, C.byref(info)) == -1
        assert b"sthip_scene_upload" in L.sthip_last_error(h)
        r.update(sc)
        before = r.render(frame, 0, 2)
        assert L.sthip_scene_update_vertices(h, None, 0, n, None) == -1
        assert b"NULL" in L.sthip_last_error(h)
        for first, count in ((0, n + 1), (n, 1), (1, n), (0xFFFFFFFF, 2)):
            assert L.sthip_scene_update_vertices(h, wire.ptr(sc.vertices), first, count, C.byref(info)) == -1, (first, count)
            assert b"vertex_count" in L.sthip_last_error(h)
        assert L.sthip_scene_update_vertices(None, wire.ptr(sc.vertices), 0, n, None) == -1
        same_frame(r.render(frame, 0, 2), before, "after the refused calls")
        assert r.stats()["full_rebuilds"] == 0
        assert L.sthip_scene_update_vertices(h, wire.ptr(sc.vertices), n, 0, C.byref(info)) == 0  # an empty range at the end is a range
        same_frame(r.render(frame, 0, 2), before, "after an empty update")
    finally:
        r.close()


# ---- the C++ host ----
@pytest.fixture(scope="module")
def deform_host(built):
    src = os.path.join(ROOT, "tests", "cpp", "deform_host.cpp")
    deps = [src, os.path.join(ROOT, "tests", "cpp", "scene_reader.hpp"), os.path.join(ROOT, "stratum_amd", "host", "stratum_hip.hpp"), os.path.join(ROOT, "include", "sthip.h")]
    if not os.path.exists(DEFORM_HOST) or os.path.getmtime(DEFORM_HOST) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(
            ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-o", DEFORM_HOST, src, "-L" + os.path.join(ROOT, "stratum_amd"), "-lstratum_hip", "-Wl,-rpath," + os.path.join(ROOT, "stratum_amd")]
        )
    return DEFORM_HOST


def test_cpp_host_with_the_vertex_update_builds(deform_host):
    """The C++ host with BDPT::update's vertices-only path, same_topology and MeshPrimitive::set_vertices compiles and links
    against the library (no GPU needed); without arguments the program only prints its usage."""
    out = subprocess.run([deform_host], capture_output=True, text=True)
    assert out.returncode == 2 and "usage: deform_host" in out.stderr


def test_cpp_multi_device_driver_uploads_a_deformed_mesh_on_every_rank(tmp_path):
    """stm::MultiDeviceBDPT over the stand-ins of tests/cpp/multi_mock.cpp (no GPU): its ranks must walk the same tree form, so a
    deformed mesh is a full upload on all of them: rank 0 does not refit (sthip_scene_update_vertices is never called) and
    last_update_was_vertices_only() stays false."""
    from stratum_amd.scene import dump_description

    exe = str(tmp_path / "multi_deform_mock")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "multi_deform_mock.cpp"), "-lpthread"])
    sc, cam = scenes.cornell_box()
    desc = str(tmp_path / "scene.bin")
    dump_description(desc, sc, camera.Frame(192, 96, cam["fovy"], cam["eye"], cam["target"]))
    out = subprocess.run([exe, desc, "3"], capture_output=True, text=True, timeout=200)
    assert out.returncode == 0 and "MULTI DEFORM OK world 3" in out.stdout, out.stdout + out.stderr[-2000:]


@pytest.mark.gpu
def test_cpp_host_deforms_a_mesh_with_a_refit(deform_host, tmp_path):
    """A MeshPrimitive deforms between two frames: Scene::update repacks, BDPT::update finds only vertex contents changed,
    calls sthip_scene_update_vertices and reports last_update_was_vertices_only(); the second frame equals, byte for byte, what
    the Python host gets from SceneData.set_vertices + BDPT.update_vertices. The displacement is y += 0.04 * (x * z) in
    binary32, the same three roundings on both sides."""
    from stratum_amd.bdpt import BDPT
    from stratum_amd.scene import dump_description

    sc, cam = scenes.cornell_box()
    W, H, seeds = 96, 64, 2
    fr = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
    desc, outp = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    dump_description(desc, sc, fr)
    out = subprocess.run([deform_host, desc, outp, str(seeds)], capture_output=True, text=True)
    assert out.returncode == 0 and "DEFORMED vertices_only=1 transforms_only=0" in out.stdout, out.stdout + out.stderr
    raw = np.fromfile(outp, dtype=np.uint8)
    rad = raw[: W * H * 16].view(np.float32).reshape(H, W, 4)
    prev_uv = raw[W * H * 16 : W * H * 24].view(np.float32).reshape(H, W, 2)
    rays = raw[W * H * 24 : W * H * 24 + 16].view(np.uint64)
    r = BDPT(device=0)
    try:
        r.update(sc)
        first = r.render(fr, 0, seeds)
        v = sc.vertices.copy()
        p = v["position"]
        p[:, 1] = p[:, 1] + np.float32(0.04) * (p[:, 0] * p[:, 2])
        sc.set_vertices(0, v)
        assert r.update_vertices(sc)["rebuilt"] == 0
        ref = r.render(fr, seeds, seeds)  # the C++ host's frame number went on: seeds `seeds` .. 2 seeds - 1
    finally:
        r.close()
    assert np.array_equal(rad.view(np.uint32), ref["radiance"].view(np.uint32))
    assert np.array_equal(prev_uv.view(np.uint32), ref["prev_uv"].view(np.uint32))
    assert np.array_equal(rays, ref["ray_count"])
    assert not np.array_equal(first["radiance"], ref["radiance"])
