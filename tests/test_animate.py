"""Rigs posed on the device: sthip_scene_set_rigs keeps a rest pose, blend targets and bone weights resident,
sthip_scene_animate sends a pose (four factors, a few bone matrices), one kernel (stratum_amd/csrc/animate.hip) writes the
rigged records of gVertices and the refit of sthip_scene_update_vertices follows. The arithmetic is part of the contract
(include/sthip.h): binary32, unfused, left to right. `posed` below restates it with numpy's float32 operations, which are
correctly rounded and unfused, so every comparison here is of bits, without a tolerance."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from stratum_amd import camera, scenes, wire

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_refit import SCENES, deformed, make_renderer, mesh_range, oracle_frame, same_frame  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANIMATE_HOST = os.path.join(ROOT, "tests", "cpp", "animate_host")
f32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------------
# the reference: the three steps of include/sthip.h in numpy float32
# ---------------------------------------------------------------------------------------------------------------------------
def posed(rest, targets=(), factors=(), weights=None, bones=None):
    """The records a rig over `rest` takes in a pose. Every operation is one float32 operation, in the order of the header."""
    out = rest.copy()
    p, n = rest["position"].copy(), rest["normal"].copy()
    assert p.dtype == np.float32 and n.dtype == np.float32
    if len(targets):
        b = [f32(factors[k]) if k < len(targets) and k < len(factors) else f32(0) for k in range(4)]
        f = np.maximum(f32(0), f32(1) - (((np.abs(b[0]) + np.abs(b[1])) + np.abs(b[2])) + np.abs(b[3])))
        assert f.dtype == np.float32
        p, n = f * p, f * n
        for k, t in enumerate(targets):
            p = p + b[k] * t["position"]
            n = n + b[k] * t["normal"]
        d = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        assert (d > 0).all() and np.isfinite(d).all(), "a blended normal of zero length: choose another pose"
        inv = f32(1) / np.sqrt(d)
        n = n * inv[:, None]
    if weights is not None:
        bones = np.ascontiguousarray(bones, dtype=np.float32).reshape(-1, 3, 4)
        m = np.zeros((rest.shape[0], 3, 4), dtype=np.float32)
        for j in range(4):
            m = m + bones[weights["indices"][:, j]] * weights["weights"][:, j][:, None, None]
        q = ((m[:, :, 0] * p[:, 0:1] + m[:, :, 1] * p[:, 1:2]) + m[:, :, 2] * p[:, 2:3]) + m[:, :, 3]
        n = (m[:, :, 0] * n[:, 0:1] + m[:, :, 1] * n[:, 1:2]) + m[:, :, 2] * n[:, 2:3]
        p = q
    assert p.dtype == np.float32 and n.dtype == np.float32 and np.isfinite(p).all() and np.isfinite(n).all()
    out["position"], out["normal"] = p, n
    return out


FACTORS = (0.3, -0.2, 0.15, 0.1)


def make_rig(vertices, first, count, n_targets, bone_count, seed):
    """(rig, pose, the posed records) over vertices[first : first + count]: targets are smooth deformations of the rest pose,
    weights include zeros and repeated indices, bones are affine maps near the identity."""
    rng = np.random.default_rng(seed)
    rest = vertices[first : first + count].copy()
    targets = [deformed(rest, 0.05 + 0.02 * k, freq=2.0 + k, phase=0.3 * k + 0.1 * seed) for k in range(n_targets)]
    rig = {"first_vertex": first, "vertex_count": count, "blend_targets": targets, "bone_count": bone_count}
    pose = {"blend_factors": FACTORS[:n_targets]}
    weights = bones = None
    if bone_count:
        weights = np.zeros(count, dtype=wire.VertexWeight)
        w = rng.random((count, 4)).astype(np.float32)
        w[rng.random((count, 4)) < 0.3] = 0  # weights of zero
        w[:, 0] = np.maximum(w[:, 0], f32(0.25))
        weights["weights"] = w / w.sum(axis=1, keepdims=True, dtype=np.float32)
        idx = rng.integers(0, bone_count, (count, 4)).astype(np.uint32)
        repeat = rng.random(count) < 0.3  # the same bone twice
        idx[repeat, 1] = idx[repeat, 0]
        idx[0] = bone_count - 1  # the last bone is used
        weights["indices"] = idx
        bones = np.zeros((bone_count, 3, 4), dtype=np.float32)
        bones[:, :, :3] = np.eye(3, dtype=np.float32) + (0.08 * rng.standard_normal((bone_count, 3, 3))).astype(np.float32)
        bones[:, :, 3] = (0.04 * rng.standard_normal((bone_count, 3))).astype(np.float32)
        rig["weights"] = weights
        pose["bones"] = bones
    return rig, pose, posed(rest, targets, FACTORS[:n_targets], weights, bones)


def bits(v):
    return np.ascontiguousarray(v).view(np.uint32)


def apply(sc, rigs_and_expected):
    """The posed records into a scene (the host's way to the same vertices)."""
    for rig, _, expected in rigs_and_expected:
        if rig["vertex_count"]:
            sc.set_vertices(rig["first_vertex"], expected)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
NAMES = ("sthip_scene_set_rigs", "sthip_scene_animate", "sthip_scene_read_vertices")


def test_library_exports_the_rig_calls(built):
    from stratum_amd import _lib

    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name), name
    assert _lib.lib().sthip_abi_version() == 11


def test_header_declares_the_rig_calls():
    text = open(os.path.join(ROOT, "include", "sthip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int\s+sthip_scene_set_rigs\s*\(\s*sthip_ctx\s*\*\s*\w*\s*,\s*const\s+sthip_rig_desc\s*\*\s*\w*\s*,\s*uint32_t\s+\w+\s*\)", text)
    assert re.search(r"int\s+sthip_scene_animate\s*\(\s*sthip_ctx\s*\*\s*\w*\s*,\s*const\s+sthip_rig_pose\s*\*\s*\w*\s*,\s*uint32_t\s+\w+\s*,\s*sthip_refit_info\s*\*\s*\w*\s*\)", text)
    assert re.search(r"int\s+sthip_scene_read_vertices\s*\(\s*sthip_ctx\s*\*\s*\w*\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*sthip_PackedVertexData\s*\*\s*\w*\s*\)", text)
    assert "typedef struct sthip_rig_desc" in text and "typedef struct sthip_rig_pose" in text
    assert "typedef struct sthip_VertexWeight" in open(os.path.join(ROOT, "include", "sthip_wire.h")).read()
    assert re.search(r"#define\s+STHIP_ABI_VERSION\s+11\b", text)


def test_mirrors_have_the_sizes_of_the_c_structs(built, tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "sthip.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(sthip_VertexWeight), sizeof(sthip_rig_desc), sizeof(sthip_rig_pose)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)])
    sizes = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert sizes == [wire.VertexWeight.itemsize, C.sizeof(wire.RigDesc), C.sizeof(wire.RigPose)] == [wire.VERTEX_WEIGHT_BYTES, wire.RIG_DESC_BYTES, wire.RIG_POSE_BYTES]
    assert [f for f, _ in wire.RigDesc._fields_] == ["first_vertex", "vertex_count", "blend_target_count", "bone_count", "blend_targets", "weights"]
    assert [f for f, _ in wire.RigPose._fields_] == ["blend_factors", "bones"]
    assert wire.VertexWeight.names == ("weights", "indices")


def test_the_numpy_statement_on_values_worked_by_hand():
    """The reference itself: one vertex, numbers that are exact in binary32."""
    rest = np.zeros(1, dtype=wire.PackedVertexData)
    rest["position"], rest["normal"], rest["u"], rest["v"] = (1, 2, 4), (0, 0, 2), 0.25, 0.75
    t = rest.copy()
    t["position"], t["normal"] = (3, 2, 0), (0, 0, 6)
    got = posed(rest, [t], [0.5])  # f = 0.5: p = 0.5 r + 0.5 t
    assert got["position"].tolist() == [[2, 2, 2]] and got["normal"].tolist() == [[0, 0, 1]] and got["u"][0] == 0.25 and got["v"][0] == 0.75
    w = np.zeros(1, dtype=wire.VertexWeight)
    w["weights"], w["indices"] = (0.5, 0.5, 0, 0), (0, 1, 1, 0)
    bones = np.zeros((2, 3, 4), dtype=np.float32)
    bones[0, :, :3], bones[1, :, :3] = np.eye(3), 3 * np.eye(3)
    bones[1, :, 3] = (2, 0, -2)
    got = posed(rest, [], [], w, bones)  # M = 2 I, translation (1, 0, -1)
    assert got["position"].tolist() == [[3, 4, 7]] and got["normal"].tolist() == [[0, 0, 4]]
    t["normal"] = (0, 0, -2)  # a pose whose blended normal vanishes is refused by the helper
    with pytest.raises(AssertionError):
        posed(rest, [t], [0.5])


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: vertices
# ---------------------------------------------------------------------------------------------------------------------------
# (first_vertex, vertex_count or None for a whole mesh, targets, bones) per rig; the forest's tree mesh is 420 records, its
# ground 32761: neither a multiple of 64 or 256. The last case lies in records appended behind the scene's own (no triangle
# refers to them): more than 256 CUs x 4 blocks x 256 lanes, so the kernel's grid-stride loop goes round.
VERTEX_CASES = {
    "blend-1-target": [(33, 63, 1, 0)],
    "blend-4-targets": [(101, 257, 4, 0)],
    "skin-1-bone-1-vertex": [(7, 1, 0, 1)],
    "skin-300-bones-whole-mesh": [("ground", None, 0, 300)],
    "both-whole-mesh": [("tree", None, 2, 5)],
    "both-300-bones": [(1001, 257, 4, 300)],
    "two-rigs-with-a-gap": [(3, 63, 1, 1), (301, 257, 0, 300)],
    "grid-stride": [("appended", 256 * 4 * 256 + 257, 1, 3)],
}
APPENDED = 256 * 4 * 256 + 300


def _forest(appended):
    sc, cam = SCENES["forest"][0]()
    own = sc.vertices.shape[0]
    if appended:
        extra = np.zeros(APPENDED, dtype=wire.PackedVertexData)
        rng = np.random.default_rng(5)
        extra["position"] = rng.uniform(-3, 3, (APPENDED, 3)).astype(np.float32)
        normal = rng.standard_normal((APPENDED, 3))
        extra["normal"] = (normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(np.float32)
        extra["u"], extra["v"] = rng.random(APPENDED).astype(np.float32), rng.random(APPENDED).astype(np.float32)
        sc.vertices = np.concatenate([sc.vertices, extra])
    return sc, cam, own


def _rigs_of(sc, own, case):
    out = []
    for seed, (first, count, n_targets, bone_count) in enumerate(VERTEX_CASES[case]):
        if first == "ground":
            first, count = mesh_range(sc, 0)
        elif first == "tree":
            first, count = mesh_range(sc, 1)
        elif first == "appended":
            first = own + 12
        out.append(make_rig(sc.vertices, first, count, n_targets, bone_count, seed + 1))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(VERTEX_CASES))
def test_vertices_equal_the_numpy_statement(built, case):
    """After set_rigs and animate the resident records equal the numpy statement bit for bit over the rigged ranges and the
    uploaded records everywhere else; u and v are the rest pose's."""
    sc, _, own = _forest(case == "grid-stride")
    rigs = _rigs_of(sc, own, case)
    for rig, _, _ in rigs:
        assert rig["vertex_count"] % 64 and rig["first_vertex"] + rig["vertex_count"] <= sc.vertices.shape[0]
    assert case == "skin-300-bones-whole-mesh" or all(rig["first_vertex"] % 2 == 1 for rig, _, _ in rigs)  # (the ground starts at record 0)
    r = make_renderer(options={"bvh_builder": 1})
    try:
        r.update(sc)
        n = sc.vertices.shape[0]
        assert np.array_equal(bits(r.read_vertices(0, n)), bits(sc.vertices))
        r.set_rigs([rig for rig, _, _ in rigs])
        info = r.animate([pose for _, pose, _ in rigs])
        assert info["rebuilt"] == 0 and info["device_ms"] > 0
        expected = sc.vertices.copy()
        for rig, _, records in rigs:
            expected[rig["first_vertex"] : rig["first_vertex"] + rig["vertex_count"]] = records
        got = r.read_vertices(0, n)
        changed = np.flatnonzero((bits(expected).reshape(n, 8) != bits(sc.vertices).reshape(n, 8)).any(axis=1))
        assert changed.size >= sum(rig["vertex_count"] for rig, _, _ in rigs) * 0.9  # (the pose moves things)
        wrong = np.flatnonzero((bits(got).reshape(n, 8) != bits(expected).reshape(n, 8)).any(axis=1))
        assert wrong.size == 0, (case, wrong[:8], got[wrong[:2]], expected[wrong[:2]])
        part = r.read_vertices(rigs[0][0]["first_vertex"], rigs[0][0]["vertex_count"])
        assert np.array_equal(bits(part), bits(rigs[0][2]))
    finally:
        r.close()


@pytest.mark.gpu
def test_vertices_with_poisoned_allocations(built):
    """The vertex cases once more in a fresh child process with STHIP_POISON_ALLOC (read once per process): rest poses,
    targets, weights and bones start as 0x7F bytes, so a record or a bone the kernel reads before anything wrote it shows."""
    if os.environ.get("STHIP_ANIMATE_POISON_CHILD"):
        return  # (this is the child)
    env = dict(os.environ, STHIP_POISON_ALLOC="0x7F", STHIP_ANIMATE_POISON_CHILD="1")
    out = subprocess.run(
        [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "vertices_equal or chain_of_three"],
        env=env, cwd=ROOT, capture_output=True, text=True, timeout=600,
    )
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "failed" not in out.stdout


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: frames
# ---------------------------------------------------------------------------------------------------------------------------
# per scene: (instance whose mesh is rigged, targets, bones) — cornell: the floor (part of the merged mesh) and the mesh the
# two boxes share; forest: a tree mesh shared by transformed instances and the ground; textured: the textured mesh
FRAME_RIGS = {"cornell": [(0, 2, 0), (5, 1, 3)], "forest": [(1, 2, 4), (0, 0, 2)], "textured": [(5, 1, 2)]}


def _scene_rigs(sc, spec):
    return [make_rig(sc.vertices, *mesh_range(sc, instance), n_targets, bone_count, 10 + k) for k, (instance, n_targets, bone_count) in enumerate(spec)]


@pytest.mark.gpu
@pytest.mark.parametrize("builder", [0, 1])
@pytest.mark.parametrize("name", sorted(FRAME_RIGS))
def test_animate_gives_the_frame_of_the_host_path_of_a_fresh_upload_and_of_the_oracle(built, name, builder):
    make, args, flags = SCENES[name]
    sc, cam = make()
    rigs = _scene_rigs(sc, FRAME_RIGS[name])
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    r = make_renderer(args, flags, {"bvh_builder": builder})
    other = make_renderer(args, flags, {"bvh_builder": builder})
    try:
        r.update(sc)
        before = r.render(frame, 0, 2)
        r.set_rigs([rig for rig, _, _ in rigs])
        rebuilds = r.stats()["full_rebuilds"]
        info = r.animate([pose for _, pose, _ in rigs])
        print(name, builder, info)
        assert info["rebuilt"] == 0 and r.stats()["full_rebuilds"] == rebuilds
        assert info["sah_cost"] > 0 and info["sah_cost_at_build"] > 0 and info["device_ms"] > 0
        got = r.render(frame, 0, 2)
        assert not np.array_equal(before["radiance"], got["radiance"])
        ref, _ = make()
        other.update(ref)
        apply(ref, rigs)
        assert other.update_vertices(ref)["rebuilt"] == 0
        same_frame(got, other.render(frame, 0, 2), "(a) the numpy vertices through update_vertices")
        other.update(ref)
        same_frame(got, other.render(frame, 0, 2), "(b) a fresh upload of the numpy vertices")
        same_frame(got, oracle_frame(ref, r, frame, 0, 2), "(c) the oracle")
    finally:
        r.close()
        other.close()


def _fresh_frame(sc, frame, options=None, seeds=(0, 2)):
    r = make_renderer(options=options)
    try:
        r.update(sc)
        return r.render(frame, *seeds)
    finally:
        r.close()


@pytest.mark.gpu
def test_a_rig_on_an_emissive_mesh_moves_the_emitter_bounds(built):
    """answer_last_rays on: the bounds last rays are aimed at follow the posed light."""
    sc, cam = scenes.cornell_box()
    light = int(sc.lights[0])
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    first, count = mesh_range(sc, light)
    rig = {"first_vertex": first, "vertex_count": count, "bone_count": 1, "weights": np.zeros(count, dtype=wire.VertexWeight)}
    rig["weights"]["weights"][:, 0] = 1
    bone = np.zeros((1, 3, 4), dtype=np.float32)
    bone[0, :, :3] = np.eye(3, dtype=np.float32) * f32(0.75)
    bone[0, :, 3] = (0.1, -0.125, 0.05)
    expected = posed(sc.vertices[first : first + count], weights=rig["weights"], bones=bone)
    r = make_renderer(options={"answer_last_rays": 1})
    try:
        r.update(sc)
        before = r.render(frame, 0, 2)
        r.set_rigs([rig])
        assert r.animate([{"bones": bone}])["rebuilt"] == 0
        got = r.render(frame, 0, 2)
        assert r.stats()["rays_answered"] > 0
        assert not np.array_equal(before["radiance"], got["radiance"])
        sc.set_vertices(first, expected)
        same_frame(got, _fresh_frame(sc, frame, {"answer_last_rays": 1}), "a fresh upload")
        r.set_option("answer_last_rays", 0)
        same_frame(got, r.render(frame, 0, 2), "every last ray traced")
    finally:
        r.close()


@pytest.mark.gpu
def test_rigs_survive_an_upload_refused_by_its_check(built):
    """An upload that check_scene refuses leaves the context as it was: the rigs set before it still pose the resident scene, and
    the frame is the one the same pose gives without the refused call in between."""
    from stratum_amd._lib import StratumHipError

    sc, cam = scenes.cornell_box()
    frame = camera.Frame(32, 32, cam["fovy"], cam["eye"], cam["target"])
    rigs = _scene_rigs(sc, [(0, 2, 0)])  # the floor
    frames = []
    for refused in (False, True):
        r = make_renderer()
        try:
            r.update(sc)
            r.set_rigs([rig for rig, _, _ in rigs])
            if refused:
                bad, _ = scenes.cornell_box()
                bad.lights[0] = bad.instances.shape[0]
                with pytest.raises(StratumHipError, match="gLightInstances entry out of range"):
                    r.update(bad)
            assert r.animate([pose for _, pose, _ in rigs])["rebuilt"] == 0
            frames.append({k: v.copy() for k, v in r.render(frame, 0, 1).items()})
        finally:
            r.close()
    same_frame(frames[1], frames[0], "the pose without the refused upload")


@pytest.mark.gpu
def test_chain_of_three_poses_is_the_last_pose_alone(built):
    """A pose is a function of the rest pose, not of the poses before it."""
    sc, cam = scenes.cornell_box()
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    rig, pose, expected = _scene_rigs(sc, [(5, 2, 3)])[0]
    poses = [dict(pose, blend_factors=(0.1 * k, 0.2), bones=pose["bones"] * f32(1 + 0.05 * k)) for k in (1, 2)] + [pose]
    r, alone = make_renderer(), make_renderer()
    try:
        r.update(sc)
        r.set_rigs([rig])
        for p in poses:
            assert r.animate([p])["rebuilt"] == 0
        alone.update(sc)
        alone.set_rigs([rig])
        alone.animate([pose])
        n = sc.vertices.shape[0]
        assert np.array_equal(bits(r.read_vertices(0, n)), bits(alone.read_vertices(0, n)))
        assert np.array_equal(bits(r.read_vertices(rig["first_vertex"], rig["vertex_count"])), bits(expected))
        same_frame(r.render(frame, 0, 2), alone.render(frame, 0, 2), "three poses against the last alone")
    finally:
        r.close()
        alone.close()


@pytest.mark.gpu
def test_identity_pose_leaves_the_positions_of_the_rest_pose(built):
    """Factors 0, one identity bone with weight 1: 1 * x + 0 * y + 0 * z + 0 is x (no coordinate of the mesh is -0, whose sign
    the sum with +0 would lose), and the frame is the rest pose's."""
    sc, cam = scenes.cornell_box()
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    first, count = mesh_range(sc, 5)
    rest = sc.vertices[first : first + count].copy()
    assert not np.signbit(rest["position"][rest["position"] == 0]).any()
    weights = np.zeros(count, dtype=wire.VertexWeight)
    weights["weights"][:, 0] = 1
    bone = np.zeros((1, 3, 4), dtype=np.float32)
    bone[0, :, :3] = np.eye(3, dtype=np.float32)
    r = make_renderer()
    try:
        r.update(sc)
        before = r.render(frame, 0, 2)
        r.set_rigs([{"first_vertex": first, "vertex_count": count, "bone_count": 1, "weights": weights}])
        assert r.animate([{"blend_factors": (0, 0, 0, 0), "bones": bone}])["rebuilt"] == 0
        got = r.read_vertices(first, count)
        assert np.array_equal(bits(got["position"]), bits(rest["position"]))
        assert np.array_equal(bits(got), bits(posed(rest, weights=weights, bones=bone)))
        assert np.array_equal(got["normal"], rest["normal"])  # (as values: -0 may have become +0)
        same_frame(r.render(frame, 0, 2), before, "the identity pose")
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the kept scene
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", [{"wide_bvh": 3}, {"embed_leaves": 1}], ids=["wide_bvh-3", "embed_leaves"])
def test_layouts_the_refit_does_not_serve_are_built_again(built, layout):
    """The kernel runs, the ranges are read back into the kept scene and the scene is built again from it; twice, so the
    rigs outlive the rebuild. With keep_scene = 0 the call is refused as unsupported and nothing changes."""
    from stratum_amd._lib import StratumHipError

    sc, cam = scenes.cornell_box()
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    rigs = _scene_rigs(sc, FRAME_RIGS["cornell"])
    r = make_renderer(options=layout)
    try:
        r.update(sc)
        r.set_rigs([rig for rig, _, _ in rigs])
        rebuilds = r.stats()["full_rebuilds"]
        half = [dict(pose, blend_factors=(0.05,) * len(pose["blend_factors"])) for _, pose, _ in rigs]
        assert r.animate(half)["rebuilt"] == 1
        info = r.animate([pose for _, pose, _ in rigs])
        assert info["rebuilt"] == 1 and r.stats()["full_rebuilds"] == rebuilds + 2
        got = r.render(frame, 0, 2)
        ref, _ = scenes.cornell_box()
        apply(ref, rigs)
        same_frame(got, _fresh_frame(ref, frame, layout), "(b) a fresh upload, " + str(layout))
    finally:
        r.close()
    r = make_renderer(options=dict(layout, keep_scene=0))
    try:
        r.update(sc)
        before = r.render(frame, 0, 2)
        r.set_rigs([rig for rig, _, _ in rigs])
        with pytest.raises(StratumHipError) as e:
            r.animate([pose for _, pose, _ in rigs])
        assert "(-4)" in str(e.value) and "keep_scene" in str(e.value)  # STHIP_ERR_UNSUPPORTED
        assert np.array_equal(bits(r.read_vertices(0, sc.vertices.shape[0])), bits(sc.vertices))
        same_frame(r.render(frame, 0, 2), before, "refused: the old scene")
    finally:
        r.close()


@pytest.mark.gpu
def test_a_rebuild_from_the_kept_scene_sees_the_posed_vertices(built):
    """animate, then update_transforms moves an instance of the merged mesh: the scene is built again from the kept copy,
    whose rigged ranges are read back from the device first. A host update_vertices over part of a posed range in between
    stays: the read-back does not overwrite the newer records."""
    from stratum_amd.scene import translate

    sc, cam = scenes.cornell_box()
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    rigs = _scene_rigs(sc, FRAME_RIGS["cornell"])
    r = make_renderer()
    try:
        r.update(sc)
        r.set_rigs([rig for rig, _, _ in rigs])
        assert r.animate([pose for _, pose, _ in rigs])["rebuilt"] == 0
        ref, _ = scenes.cornell_box()
        apply(ref, rigs)
        # the host writes the second half of the second rig's range
        rig = rigs[1][0]
        lo = rig["first_vertex"] + rig["vertex_count"] // 2
        part = deformed(ref.vertices[lo : rig["first_vertex"] + rig["vertex_count"]], 0.03)
        ref.set_vertices(lo, part)
        sc.set_vertices(lo, part)
        assert r.update_vertices(sc)["rebuilt"] == 0
        for s in (sc, ref):
            s.set_instance_transform(0, translate((0.0, 0.1, 0.0)))
        r.update_transforms(sc)
        assert r.stats()["full_rebuilds"] == 1
        got = r.render(frame, 0, 2)
        assert np.array_equal(bits(r.read_vertices(0, ref.vertices.shape[0])), bits(ref.vertices))
        same_frame(got, _fresh_frame(ref, frame), "a fresh upload of both changes")
        same_frame(got, oracle_frame(ref, r, frame, 0, 2), "the oracle")
        # the rigs outlived the rebuild, and their rest pose is the one they were set with
        assert r.animate([pose for _, pose, _ in rigs])["rebuilt"] == 0
        assert np.array_equal(bits(r.read_vertices(rig["first_vertex"], rig["vertex_count"])), bits(rigs[1][2]))
    finally:
        r.close()


@pytest.mark.gpu
def test_default_layout_animates_without_a_kept_scene(built):
    sc, cam = scenes.cornell_box()
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    rigs = _scene_rigs(sc, FRAME_RIGS["cornell"])
    r = make_renderer(options={"keep_scene": 0})
    try:
        r.update(sc)
        r.set_rigs([rig for rig, _, _ in rigs])
        assert r.animate([pose for _, pose, _ in rigs])["rebuilt"] == 0 and r.stats()["full_rebuilds"] == 0
        got = r.render(frame, 0, 2)
        apply(sc, rigs)
        same_frame(got, _fresh_frame(sc, frame), "keep_scene = 0")
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: refusals, frames in flight
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_invalid_arguments_are_refused_with_a_message(built):
    """Every refusal of sthip.h: -1 (STHIP_ERR_INVALID_ARGUMENT), a message, and nothing changed: the rigs set before stay
    and the frame is the one before."""
    from stratum_amd.bdpt import BDPT

    sc, cam = scenes.cornell_box()
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    n = sc.vertices.shape[0]
    r = BDPT(device=0)
    try:
        L, h = r._lib, r._h

        def refused(rc, word=None):
            assert rc == -1
            msg = L.sthip_last_error(h)
            assert msg and (word is None or word in msg), msg

        def desc(first=1, count=9, targets=0, bones=0, weights=None, target_ptrs=None):
            d = wire.RigDesc()
            d.first_vertex, d.vertex_count, d.blend_target_count, d.bone_count = first, count, targets, bones
            for k, t in enumerate(target_ptrs or []):
                d.blend_targets[k] = t.ctypes.data if t is not None else None
            d.weights = weights.ctypes.data if weights is not None else None
            return d

        def set_rigs(*descs):
            return L.sthip_scene_set_rigs(h, (wire.RigDesc * len(descs))(*descs), len(descs))

        target = sc.vertices[1:10].copy()
        weights = np.zeros(9, dtype=wire.VertexWeight)
        weights["weights"][:, 0] = 1
        pose = wire.RigPose()
        refused(set_rigs(desc()), b"sthip_scene_upload")  # no scene
        refused(L.sthip_scene_animate(h, C.byref(pose), 1, None), b"sthip_scene_upload")
        r.update(sc)
        before = r.render(frame, 0, 2)
        refused(L.sthip_scene_animate(h, C.byref(pose), 1, None), b"sthip_scene_set_rigs")  # no rigs
        refused(set_rigs(desc(first=n - 4, count=5)), b"vertex_count")
        refused(set_rigs(desc(first=0xFFFFFFFF, count=2)), b"vertex_count")
        refused(set_rigs(desc(first=1, count=9), desc(first=9, count=3)), b"overlap")
        refused(set_rigs(desc(targets=5, target_ptrs=[target] * 4)), b"blend_target_count")
        refused(set_rigs(desc(bones=1025, weights=weights)), b"bone_count")
        refused(set_rigs(desc(targets=2, target_ptrs=[target, None])), b"NULL")
        refused(set_rigs(desc(bones=2)), b"NULL")
        refused(L.sthip_scene_set_rigs(h, None, 1), b"NULL")
        bad = weights.copy()
        bad["indices"][5, 3] = 2
        refused(set_rigs(desc(bones=2, weights=bad)), b"bone index")
        refused(L.sthip_scene_animate(h, C.byref(pose), 1, None), b"sthip_scene_set_rigs")  # (none of them left a rig behind)
        # a good rig; then refused poses, and a refused set_rigs that must leave it in place
        assert set_rigs(desc(targets=1, target_ptrs=[target], bones=2, weights=weights)) == 0
        bones = np.zeros((2, 3, 4), dtype=np.float32)
        bones[:, :, :3] = np.eye(3, dtype=np.float32)
        pose.bones = bones.ctypes.data
        refused(L.sthip_scene_animate(h, (wire.RigPose * 2)(pose, pose), 2, None), b"pose_count")
        refused(L.sthip_scene_animate(h, C.byref(pose), 0, None), b"pose_count")
        refused(L.sthip_scene_animate(h, None, 1, None), b"NULL")
        for value in (np.inf, np.nan):
            pose.blend_factors[0] = value
            refused(L.sthip_scene_animate(h, C.byref(pose), 1, None), b"finite")
            pose.blend_factors[0] = 0
            bones[1, 2, 3] = value
            refused(L.sthip_scene_animate(h, C.byref(pose), 1, None), b"finite")
            bones[1, 2, 3] = 0
        pose.bones = None
        refused(L.sthip_scene_animate(h, C.byref(pose), 1, None), b"NULL")
        assert L.sthip_scene_set_rigs(None, None, 0) == -1 and L.sthip_scene_animate(None, None, 0, None) == -1 and L.sthip_scene_read_vertices(None, 0, 0, None) == -1
        refused(L.sthip_scene_read_vertices(h, n, 1, wire.ptr(sc.vertices)), b"vertex_count")
        refused(L.sthip_scene_read_vertices(h, 0, 1, None), b"NULL")
        refused(set_rigs(desc(first=n, count=1)), b"vertex_count")
        assert np.array_equal(bits(r.read_vertices(0, n)), bits(sc.vertices))
        same_frame(r.render(frame, 0, 2), before, "after the refused calls")
        assert r.stats()["full_rebuilds"] == 0
        pose.bones = bones.ctypes.data  # the good rig is still there: a factor of 0.5 towards the rest pose itself, identity bones
        pose.blend_factors[0] = 0.5
        assert L.sthip_scene_animate(h, C.byref(pose), 1, None) == 0
        assert np.array_equal(bits(r.read_vertices(1, 9)), bits(posed(sc.vertices[1:10], [target], [0.5], weights, bones)))
        # an upload drops the rigs; so does rig_count = 0
        r.update(sc)
        refused(L.sthip_scene_animate(h, C.byref(pose), 1, None), b"sthip_scene_set_rigs")
        assert set_rigs(desc(bones=2, weights=weights)) == 0 and L.sthip_scene_set_rigs(h, None, 0) == 0
        refused(L.sthip_scene_animate(h, C.byref(pose), 1, None), b"sthip_scene_set_rigs")
        same_frame(r.render(frame, 0, 2), before, "after the upload")
    finally:
        r.close()


@pytest.mark.gpu
def test_a_frame_in_flight_completes_with_the_pose_before(built):
    sc, cam = scenes.cornell_box()
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    rigs = _scene_rigs(sc, FRAME_RIGS["cornell"])
    r = make_renderer(options={"bvh_builder": 1})
    try:
        r.update(sc)
        r.set_rigs([rig for rig, _, _ in rigs])
        old = r.render(frame, 0, 2)
        ticket = r.render_async(frame, 0, 2)
        assert r.animate([pose for _, pose, _ in rigs])["rebuilt"] == 0
        same_frame(r.wait(ticket), old, "the ticket in flight")
        new = r.wait(r.render_async(frame, 0, 2))
        assert not np.array_equal(new["radiance"], old["radiance"])
        same_frame(new, r.render(frame, 0, 2), "async against sync")
        apply(sc, rigs)
        same_frame(new, _fresh_frame(sc, frame, {"bvh_builder": 1}), "a fresh upload")
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the C++ host
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def animate_host(built):
    src = os.path.join(ROOT, "tests", "cpp", "animate_host.cpp")
    deps = [src, os.path.join(ROOT, "tests", "cpp", "scene_reader.hpp"), os.path.join(ROOT, "stratum_amd", "host", "stratum_hip.hpp"), os.path.join(ROOT, "include", "sthip.h")]
    if not os.path.exists(ANIMATE_HOST) or os.path.getmtime(ANIMATE_HOST) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(
            ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-o", ANIMATE_HOST, src, "-L" + os.path.join(ROOT, "stratum_amd"), "-lstratum_hip", "-Wl,-rpath," + os.path.join(ROOT, "stratum_amd")]
        )
    return ANIMATE_HOST


def _host_rig(vertices):
    """The rig tests/cpp/animate_host.cpp gives every mesh, as one rig over all records (it depends on a record's own
    contents only): one target, y += 0.04 * (x * z); bones 0 (identity) and 1, weights 0.75 and 0.25; factor 0.5."""
    target = vertices.copy()
    p = target["position"]
    p[:, 1] = p[:, 1] + f32(0.04) * (p[:, 0] * p[:, 2])
    weights = np.zeros(vertices.shape[0], dtype=wire.VertexWeight)
    weights["weights"][:, :2] = (0.75, 0.25)
    weights["indices"][:] = (0, 1, 1, 0)
    bones = np.zeros((2, 3, 4), dtype=np.float32)
    bones[:, :, :3] = np.eye(3, dtype=np.float32)
    bones[1, :, :3] *= f32(0.875)
    bones[1, :, 3] = (0.0625, 0.0, 0.03125)
    return target, weights, bones, (0.5, 0.0, 0.0, 0.0)


def test_cpp_host_with_rigs_builds(animate_host):
    """The C++ host with MeshPrimitive::set_rig / set_pose and BDPT::update's pose-only path compiles and links against the
    library (no GPU needed); without arguments the program only prints its usage."""
    out = subprocess.run([animate_host], capture_output=True, text=True)
    assert out.returncode == 2 and "usage: animate_host" in out.stderr


def test_cpp_host_poses_on_the_host_with_the_arithmetic_of_the_device(animate_host, tmp_path):
    """`animate_host --host-pose` packs a scene with Scene::set_pose_on_device(false), the path for a library without
    sthip_scene_animate and for the multi-device driver: its vertices must be the numpy statement's, bit for bit."""
    from stratum_amd.scene import dump_description

    sc, cam = scenes.cornell_box()
    desc, outp = str(tmp_path / "scene.bin"), str(tmp_path / "vertices.bin")
    dump_description(desc, sc, camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"]))
    out = subprocess.run([animate_host, "--host-pose", desc, outp], capture_output=True, text=True)
    assert out.returncode == 0 and "HOST POSED" in out.stdout, out.stdout + out.stderr
    got = np.fromfile(outp, dtype=wire.PackedVertexData)
    target, weights, bones, factors = _host_rig(sc.vertices)
    expected = posed(sc.vertices, [target], factors, weights, bones)
    assert got.shape == expected.shape and np.array_equal(bits(got), bits(expected))


@pytest.mark.gpu
def test_cpp_host_poses_a_rig_on_the_device(animate_host, tmp_path):
    """Every MeshPrimitive gets a rig before the first frame and a pose after it: BDPT::update sends the rigs once after the
    upload, finds only poses changed, calls sthip_scene_animate and reports last_update_was_vertices_only(); the second frame
    equals, byte for byte, the Python host's."""
    from stratum_amd.bdpt import BDPT
    from stratum_amd.scene import dump_description

    sc, cam = scenes.cornell_box()
    W, H, seeds = 96, 64, 2
    fr = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
    desc, outp = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    dump_description(desc, sc, fr)
    out = subprocess.run([animate_host, desc, outp, str(seeds)], capture_output=True, text=True)
    assert out.returncode == 0 and "ANIMATED vertices_only=1 transforms_only=0" in out.stdout, out.stdout + out.stderr
    raw = np.fromfile(outp, dtype=np.uint8)
    rad = raw[: W * H * 16].view(np.float32).reshape(H, W, 4)
    prev_uv = raw[W * H * 16 : W * H * 24].view(np.float32).reshape(H, W, 2)
    rays = raw[W * H * 24 : W * H * 24 + 16].view(np.uint64)
    target, weights, bones, factors = _host_rig(sc.vertices)
    r = BDPT(device=0)
    try:
        r.update(sc)
        first = r.render(fr, 0, seeds)
        r.set_rigs([{"first_vertex": 0, "vertex_count": sc.vertices.shape[0], "blend_targets": [target], "weights": weights, "bone_count": 2}])
        assert r.animate([{"blend_factors": factors, "bones": bones}])["rebuilt"] == 0
        ref = r.render(fr, seeds, seeds)  # the C++ host's frame number went on: seeds `seeds` .. 2 seeds - 1
    finally:
        r.close()
    assert np.array_equal(rad.view(np.uint32), ref["radiance"].view(np.uint32))
    assert np.array_equal(prev_uv.view(np.uint32), ref["prev_uv"].view(np.uint32))
    assert np.array_equal(rays, ref["ray_count"])
    assert not np.array_equal(first["radiance"], ref["radiance"])
