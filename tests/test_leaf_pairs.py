"""Leaf records of the 4-wide tree ("leaf_pairs", stratum_amd/csrc/bvh.h: LeafPair): k_trace tests a leaf from one 64-byte
record instead of one BvhTri per triangle. The record holds the triangles' own vertices in their own order and the kernel
runs the same arithmetic on them, so a frame with leaf_pairs = 1 equals the frame with leaf_pairs = 0 on the same tree bit
for bit: radiance, every AOV, the ray counts and, with count_traversal, the number of triangles tested."""
import os
import subprocess
import sys

import numpy as np
import pytest

from stratum_amd import camera, scenes
from stratum_amd.scene import SceneBuilder

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_animate import make_rig  # noqa: E402
from test_refit import deform, make_renderer, mesh_range  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 96, 64


def few_triangles(n):
    """n triangles in front of the camera: a fan folded over itself (its halves overlap in one plane), then loose ones."""
    b = SceneBuilder("few_triangles_%d" % n)
    white = b.add_material((0.7, 0.7, 0.7))
    light = b.add_emitter((9.0, 9.0, 9.0))
    pos = [(-0.8, -0.6, 0.0), (0.6, -0.6, 0.0), (-0.8, 0.7, 0.0), (0.45, -0.45, 0.0)]
    tri = [(0, 1, 2), (0, 2, 3)][: min(n, 2)]
    for k in range(2, n):
        base = len(pos)
        x = -0.9 + 0.31 * (k - 2)
        pos += [(x, 0.75, 0.1 * k), (x + 0.3, 0.75, 0.1 * k), (x, 0.95, 0.1 * k)]
        tri.append((base, base + 1, base + 2))
    pos = np.array(pos, np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (pos.shape[0], 1))
    uv = np.zeros((pos.shape[0], 2), np.float32)
    b.add_instance(b.add_mesh(pos, nrm, uv, np.array(tri)), white)
    lp = np.array([(-0.3, 1.5, 1.0), (0.3, 1.5, 1.0), (0.3, 1.5, 1.6), (-0.3, 1.5, 1.6)], np.float32)
    b.add_instance(b.add_mesh(lp, np.tile(np.array([0, -1, 0], np.float32), (4, 1)), np.zeros((4, 2), np.float32), np.array([(0, 1, 2), (0, 2, 3)])), light)
    return b.build(), {"eye": (0.0, 0.0, 3.0), "target": (0.0, 0.0, 0.0), "fovy": np.radians(45.0)}


def strip_surface():
    """A wavy sheet whose triangles come as (c, b, a), (d, c, a) — the strip pattern — under a light."""
    b = SceneBuilder("strip_surface")
    white = b.add_material((0.7, 0.7, 0.7))
    light = b.add_emitter((9.0, 9.0, 9.0))
    scenes.add_chunked(b, scenes.grid_surface(lambda u, v: np.stack([2 * u - 1, 2 * v - 1, 0.15 * np.sin(6 * u) * np.cos(4 * v)], -1), 13, 11, flip=True), white)
    lp = np.array([(-0.3, 1.5, 1.0), (0.3, 1.5, 1.0), (0.3, 1.5, 1.6), (-0.3, 1.5, 1.6)], np.float32)
    b.add_instance(b.add_mesh(lp, np.tile(np.array([0, -1, 0], np.float32), (4, 1)), np.zeros((4, 2), np.float32), np.array([(0, 1, 2), (0, 2, 3)])), light)
    return b.build(), {"eye": (0.0, 0.0, 3.0), "target": (0.0, 0.0, 0.0), "fovy": np.radians(45.0)}


def _cornell_rig(sc):
    return make_rig(sc.vertices, *mesh_range(sc, 5), 1, 2, 7)


def _deform_then_pose(r, sc):
    """One refit from new vertex records, then one blend-shape / skinning update of the mesh the two blocks share."""
    deform(sc, 0.03, *mesh_range(sc, 0))
    assert r.update_vertices(sc)["rebuilt"] == 0
    rig, pose, _ = _cornell_rig(sc)
    r.set_rigs([rig])
    assert r.animate([pose])["rebuilt"] == 0


# alpha masks: no instantiation reads records; a refit and a device build leave none
NO_RECORDS = ("foliage_alpha", "deformed_and_posed", "device_built")


def _move_instances(r, sc):
    """A transforms-only update: the top level and the wide form are made again, the leaf triangles and their records stay."""
    from stratum_amd.scene import translate

    for i in (5, 6):  # the two blocks
        m = np.vstack([sc.transforms["m"][i], [0, 0, 0, 1]]).astype(np.float64)
        m = translate((0.05, 0.0, -0.04)) @ m
        sc.transforms["m"][i] = m[:3].astype(np.float32)
        sc.inverse_transforms["m"][i] = np.linalg.inv(m)[:3].astype(np.float32)
    r.update_transforms(sc)


# name: (scene, renderer args, flags, options set before the upload, what happens after the upload)
CASES = {
    "cornell": (scenes.cornell_box, {}, [], {}, None),  # every leaf is the two halves of a quad
    "clustered": (lambda: scenes.clustered_box(n_coincident=700, n_cluster=500), {}, [], {}, None),  # coincident triangles: ties by id within and across leaves
    "spheres_room": (scenes.spheres_room, {"maxDiffuseVertices": 3}, [], {}, None),  # entries beside the leaves
    "transformed_instances": (lambda: scenes.forest(n_instances=30, tree_tris=600, tree_kinds=2), {}, [], {}, None),  # id_bits
    "foliage_alpha": (scenes.foliage, {}, ["alphatest"], {}, None),  # the ALPHA instantiations have no record path
    "deformed_and_posed": (scenes.cornell_box, {}, [], {}, _deform_then_pose),
    "device_built": (lambda: scenes.forest(n_instances=30, tree_tris=600, tree_kinds=2), {}, [], {"bvh_builder": 1}, None),
    "strips": (strip_surface, {}, [], {}, None),
    "moved_instances": (scenes.cornell_box, {}, [], {}, _move_instances),
    "one_triangle": (lambda: few_triangles(1), {}, [], {}, None),
    "odd_count": (lambda: few_triangles(5), {}, [], {}, None),
    "bounded_stack": (scenes.cornell_box, {}, [], {"lds_stack_levels": 4}, None),  # k_trace_deep traces the overflowed rays again
}


def _frames(name, leaf_pairs):
    make, args, flags, options, after = CASES[name]
    sc, cam = make()
    frame = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
    r = make_renderer(args, flags, dict(options, leaf_pairs=leaf_pairs))
    try:
        r.update(sc)
        if after:
            after(r, sc)
        plain = r.render(frame, 0, 2)
        r.set_option("count_traversal", 1)
        counted = r.render(frame, 0, 2)
        stats = r.stats()
        return plain, counted, {k: stats[k] for k in ("rays_total", "tris_tested", "tris_tested_shadow", "leaf_records")}
    finally:
        r.close()


def _same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_frames_with_and_without_leaf_records_are_identical(built, name):
    on, on_counted, on_stats = _frames(name, 1)
    off, off_counted, off_stats = _frames(name, 0)
    print(name, on_stats, off_stats)
    _same(on, off, name)
    _same(on_counted, off_counted, name + " (count_traversal)")
    _same(on, on_counted, name + " (counting changes nothing)")
    # the record path ran where it is meant to and nowhere else (sthip_stats::leaf_records)
    assert off_stats["leaf_records"] == 0 and on_stats["leaf_records"] == (0 if name in NO_RECORDS else 1), (name, on_stats, off_stats)
    assert on_stats["rays_total"] == off_stats["rays_total"] > 0 and on_stats["tris_tested"] == off_stats["tris_tested"]
    # (an occlusion ray that the first record of a split leaf — two triangles that fit no pattern — stops is done; the loop
    # over BvhTri tests the leaf's second triangle all the same)
    assert on_stats["tris_tested_shadow"] <= off_stats["tris_tested_shadow"]
    assert np.isfinite(on["radiance"].astype(np.float32)).all() and on["radiance"][..., :3].max() > 0


@pytest.mark.gpu
def test_the_option_switches_on_a_resident_tree(built):
    """leaf_pairs acts at the next render, on the tree that is resident: 1, 0, 1 give one frame."""
    sc, cam = scenes.cornell_box()
    frame = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
    r = make_renderer()
    try:
        r.update(sc)
        a = r.render(frame, 0, 1)
        r.set_option("leaf_pairs", 0)
        b = r.render(frame, 0, 1)
        r.set_option("leaf_pairs", 1)
        c = r.render(frame, 0, 1)
        _same(a, b, "1 -> 0")
        _same(a, c, "0 -> 1")
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the builder's records against the triangles they stand for (tests/cpp/leaf_pairs_check.cpp)
# ---------------------------------------------------------------------------------------------------------------------------
def _dump(d, sc):
    d.mkdir()
    for arr, fn in ((sc.vertices, "vertices"), (sc.indices, "indices"), (sc.instances, "instances"), (sc.transforms, "xf"), (sc.inverse_transforms, "inv_xf"), (sc.materials, "materials")):
        np.ascontiguousarray(arr).tofile(str(d / (fn + ".bin")))
    return str(d)


def _grid_10k():
    b = SceneBuilder("grid_surface")
    white = b.add_material((0.7, 0.7, 0.7))
    part = scenes.grid_surface(lambda u, v: np.stack([2 * u - 1, 0.2 * np.sin(7 * u) * np.cos(5 * v), 2 * v - 1], -1), 71, 71)  # 10082 triangles
    scenes.add_chunked(b, part, white)
    # (a flipped surface lists its triangles as (c, b, a), (d, c, a): the strip pattern where the other is the fan)
    scenes.add_chunked(b, scenes.grid_surface(lambda u, v: np.stack([2 * u - 1, 1.0 + 0.1 * np.sin(5 * v), 2 * v - 1], -1), 20, 20, flip=True), white)
    return b.build()


def test_host_builder_records_reproduce_their_triangles(tmp_path):
    """Under ASan + UBSan: every record's A and B are their BvhTri entries' vertices bit for bit and in order, the ids match, a
    one-triangle leaf never exposes B, and the leaves split into two one-triangle records are exactly those that fit no pattern."""
    exe = str(tmp_path / "leaf_pairs_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-o", exe, os.path.join(ROOT, "tests", "cpp", "leaf_pairs_check.cpp"),
                           os.path.join(ROOT, "stratum_amd", "csrc", "bvh_build.cpp"), "-lpthread"])
    grid = _grid_10k()
    assert grid.triangle_count >= 10000
    for name, sc in (("cornell", scenes.cornell_box()[0]), ("clustered", scenes.clustered_box(n_coincident=700, n_cluster=500)[0]), ("grid", grid), ("few", few_triangles(5)[0]), ("strips", strip_surface()[0])):
        env = dict(os.environ, STHIP_BUILD_THREADS="4", ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
        out = subprocess.run([exe, _dump(tmp_path / name, sc)], capture_output=True, text=True, env=env)
        print(name, out.stdout.strip())
        assert out.returncode == 0 and "LEAF PAIRS OK" in out.stdout, name + ": " + out.stdout + out.stderr[-3000:]


def test_the_two_statements_of_the_triangle_test_agree(tmp_path):
    """stratum_amd/csrc/tri_test.h: the per-vertex and per-triangle parts the record path runs give the bits of the whole test
    every other kernel runs, over random and degenerate inputs (host build, no contraction, under UBSan)."""
    exe = str(tmp_path / "tri_test_parts_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fsanitize=undefined", "-o", exe, os.path.join(ROOT, "tests", "cpp", "tri_test_parts_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "TRI TEST PARTS OK" in out.stdout, out.stdout + out.stderr[-2000:]
